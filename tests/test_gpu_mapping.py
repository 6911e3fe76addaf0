"""GPU: BasicLaserMapping replacement with a LIVE rolling map vs the oracle.

process() is compared one step at a time from an identical prior state (map cubes + transforms), which is what "poses
must match on identical sweeps" means for a stateful call.  A free-running comparison over several sweeps is reported
with a looser bound: there the two maps are built from poses that differ in the last bits, individual points land in
different 0.2 / 0.4 m voxels, and the difference feeds back (SURVEY.md §7 "threshold discontinuities")."""
import os

import numpy as np
import pytest

import oracle_py as op
from conftest import GOLDEN, POSE_TOL
from loam_velodyne_amd import loamx, synth

pytestmark = pytest.mark.gpu


def _assert_same_point_set(a, b, what, tol=2e-5, max_flips=4):
    """Map insertion + per-cube voxel re-filtering from identical state is index work: the two clouds must hold the same
    points (any order) within float rounding of the registered pose (<= 2e-5 m), up to a bounded number of voxel-boundary
    flips (a point within 1e-6 of a 0.2 / 0.4 m voxel face may fall on the other side and change two centroids)."""
    from scipy.spatial import cKDTree
    assert abs(len(a) - len(b)) <= max_flips, (what, len(a), len(b))
    if len(a) == 0 or len(b) == 0:
        return 0.0
    ta, tb = cKDTree(a[:, :3]), cKDTree(b[:, :3])
    dab, iab = tb.query(a[:, :3])
    dba, _ = ta.query(b[:, :3])
    assert int((dab > tol).sum()) <= max_flips and int((dba > tol).sum()) <= max_flips, (what, int((dab > tol).sum()), int((dba > tol).sum()))
    ok = dab <= tol
    assert np.abs(a[ok, 3] - b[iab[ok], 3]).max() < 1e-3, what       # the averaged intensity travels with the point
    return float(dab[ok].max())


def test_per_step_parity_from_identical_state(orc, small_world):
    n = 7
    poses = synth.trajectory(n)
    osr, ood, omp = op.ScanRegistration(orc), op.LaserOdometry(orc), op.LaserMapping(orc)
    worst, worst_map, n_surround = 0.0, 0.0, 0
    for k in range(n):
        sw = synth.make_sweep(small_world, "VLP-16", poses[k], poses[k + 1], seed=k, az_steps=1200)
        ood.set_features(osr.process(sw.points, sw.ring_sizes))
        ood.process()
        full_end, lc, ls, ts = ood.full_to_end(), ood.last_corner(), ood.last_surf(), ood.transform_sum
        # GPU handle seeded with the oracle's state BEFORE this step
        g = loamx.LaserMapping()
        pre_c, pre_s = omp.cloud("corner_cubes"), omp.cloud("surf_cubes")
        g.load_cubes(pre_c, pre_s)
        g.set_transform("aft", omp.transform("aft"))
        g.set_transform("bef", omp.transform("bef"))
        g.update_odometry(ts)
        omp.set_inputs(lc, ls, full_end, ts)
        assert omp.process()
        rc, gfull = g.process(lc, ls, full_end)
        assert rc == loamx.OK
        for which in ("aft", "bef", "tobe"):
            d = np.abs(omp.transform(which) - g.transform(which)).max()
            worst = max(worst, d)
            assert d < POSE_TOL, (k, which, d)
        so, sg = omp.stats(), g.stats()
        assert so["iterations"] == sg["iterations"] and so["optimized"] == sg["optimized"]
        assert so["corner_from_map"] == sg["corner_from_map"] and so["surf_from_map"] == sg["surf_from_map"]
        assert so["corner_ds"] == sg["corner_ds"] and so["surf_ds"] == sg["surf_ds"] or k == 0
        assert np.abs(omp.cloud("full_res") - gfull).max() < 2e-5   # (poses agree to ~2e-7; points are up to 45 m away)
        # map contents after insertion (BasicLaserMapping.cpp:536-577) + per-cube voxel re-filtering (:580-593): the same point
        # sets, point for point
        for name, which in (("corner_cubes", "corner"), ("surf_cubes", "surf")):
            worst_map = max(worst_map, _assert_same_point_set(g.cubes(which), omp.cloud(name), (k, name)))
        # createDownsizedMap (:242-264): the oracle publishes every fifth frame, a fresh handle on its first
        if omp.has_fresh_map():
            assert g.has_fresh_map()
            n_surround += 1
            worst_map = max(worst_map, _assert_same_point_set(g.surround(), omp.cloud("surround_ds"), (k, "surround_ds")))
    assert worst < POSE_TOL and n_surround >= 2
    print(f"worst pose difference {worst:.2e}, worst matched map-point distance {worst_map:.2e} over {n} steps")


def test_per_step_parity_hdl64_full_size(orc):
    """The live map at BASELINE's sweep size: HDL-64E revolutions (64 x 2048), an odometry frame whose origin lies more than a cube
    away (the 21 x 11 x 21 window shifts, BasicLaserMapping.cpp:311-441), map insertion + per-cube re-filtering of ~40 k features
    per sweep (:536-593) and the surround cloud (:242-264) — per step from the oracle's state."""
    world = synth.World(half_extent=125.0)
    n = 6
    poses = synth.trajectory(n)
    offset = np.array([0, 0, 0, 60.0, 0.0, -55.0], np.float32)
    osr, ood, omp = op.ScanRegistration(orc), op.LaserOdometry(orc), op.LaserMapping(orc)
    worst, worst_map, n_surround = 0.0, 0.0, 0
    for k in range(n):
        sw = synth.make_sweep(world, "HDL-64E", poses[k], poses[k + 1], seed=40 + k)
        ood.set_features(osr.process(sw.points, sw.ring_sizes))
        ood.process()
        full_end, lc, ls, ts = ood.full_to_end(), ood.last_corner(), ood.last_surf(), ood.transform_sum + offset
        g = loamx.LaserMapping()
        g.load_cubes(omp.cloud("corner_cubes"), omp.cloud("surf_cubes"))
        g.set_transform("aft", omp.transform("aft"))
        g.set_transform("bef", omp.transform("bef"))
        g.update_odometry(ts)
        omp.set_inputs(lc, ls, full_end, ts)
        assert omp.process()
        rc, gfull = g.process(lc, ls, full_end)
        assert rc == loamx.OK
        for which in ("aft", "bef", "tobe"):
            d = float(np.abs(omp.transform(which) - g.transform(which)).max())
            worst = max(worst, d)
            assert d < POSE_TOL, (k, which, d)
        so, sg = omp.stats(), g.stats()
        assert so["iterations"] == sg["iterations"] and so["optimized"] == sg["optimized"]
        assert so["corner_from_map"] == sg["corner_from_map"] and so["surf_from_map"] == sg["surf_from_map"]
        assert (so["corner_ds"] == sg["corner_ds"] and so["surf_ds"] == sg["surf_ds"]) or k == 0
        assert np.abs(omp.cloud("full_res") - gfull).max() < 1e-4          # (coordinates up to ~200 m: one float ulp is 1.5e-5)
        for name, which in (("corner_cubes", "corner"), ("surf_cubes", "surf")):
            worst_map = max(worst_map, _assert_same_point_set(g.cubes(which), omp.cloud(name), (k, name), tol=6e-5, max_flips=8))
        if omp.has_fresh_map():
            assert g.has_fresh_map()
            n_surround += 1
            worst_map = max(worst_map, _assert_same_point_set(g.surround(), omp.cloud("surround_ds"), (k, "surround_ds"), tol=6e-5, max_flips=8))
    assert n_surround >= 2 and len(omp.cloud("surf_cubes")) > 20_000
    print(f"HDL-64E live map: worst pose difference {worst:.2e}, worst matched map-point distance {worst_map:.2e}")


def test_per_step_parity_hdl32_500k_live_map(orc):
    """BASELINE configs[2] exactly: HDL-32 sweeps (32 x 2048) against a LIVE map that starts at 500,000 points (the bench's own world,
    bench.py --mode live --sensor HDL-32 --map-points 500000) — every process() from the oracle's state of the step before:
    poses within 1e-4, iteration and sub-map counts equal, the updated cubes point for point (BasicLaserMapping.cpp:266-599, :626-926)."""
    world = synth.World(half_extent=65.0)
    cm, sm = world.make_map(500_000)
    n = 5
    poses = synth.trajectory(n)
    osr, ood, omp = op.ScanRegistration(orc), op.LaserOdometry(orc), op.LaserMapping(orc)
    omp.load_cubes(cm, sm)
    worst, worst_map = 0.0, 0.0
    for k in range(n):
        sw = synth.make_sweep(world, "HDL-32", poses[k], poses[k + 1], seed=500 + k)
        ood.set_features(osr.process(sw.points, sw.ring_sizes))
        ood.process()
        full_end, lc, ls, ts = ood.full_to_end(), ood.last_corner(), ood.last_surf(), ood.transform_sum
        g = loamx.LaserMapping()
        g.load_cubes(omp.cloud("corner_cubes"), omp.cloud("surf_cubes"))
        g.set_transform("aft", omp.transform("aft"))
        g.set_transform("bef", omp.transform("bef"))
        g.update_odometry(ts)
        omp.set_inputs(lc, ls, full_end, ts)
        assert omp.process()
        rc, gfull = g.process(lc, ls, full_end)
        assert rc == loamx.OK
        for which in ("aft", "bef", "tobe"):
            d = float(np.abs(omp.transform(which) - g.transform(which)).max())
            worst = max(worst, d)
            assert d < POSE_TOL, (k, which, d)
        so, sg = omp.stats(), g.stats()
        assert so["iterations"] == sg["iterations"] and so["optimized"] == sg["optimized"]
        assert so["corner_from_map"] == sg["corner_from_map"] and so["surf_from_map"] == sg["surf_from_map"]
        assert so["corner_from_map"] + so["surf_from_map"] > 150_000          # (the sub-map is the 500 k map's part inside the field of view)
        assert so["corner_ds"] == sg["corner_ds"] and so["surf_ds"] == sg["surf_ds"]
        assert np.abs(omp.cloud("full_res") - gfull).max() < 5e-5
        for name, which in (("corner_cubes", "corner"), ("surf_cubes", "surf")):
            worst_map = max(worst_map, _assert_same_point_set(g.cubes(which), omp.cloud(name), (k, name), tol=3e-5, max_flips=8))
        g.close()
    print(f"HDL-32 / 500 k live map: worst pose difference {worst:.2e}, worst matched map-point distance {worst_map:.2e} over {n} steps")


def test_golden_steps(orc):
    g = np.load(os.path.join(GOLDEN, "mapping_seq_vlp16.npz"))
    for t in (3, 4):
        m = loamx.LaserMapping()
        m.load_cubes(g[f"pre_corner_cubes_{t}"], g[f"pre_surf_cubes_{t}"])
        m.set_transform("aft", g[f"pre_aft_{t}"])
        m.set_transform("bef", g[f"pre_bef_{t}"])
        m.update_odometry(g[f"sum_{t}"])
        rc, full = m.process(g[f"corner_last_{t}"], g[f"surf_last_{t}"], g[f"full_{t}"])
        assert rc == loamx.OK
        assert np.abs(m.transform("aft") - g[f"post_aft_{t}"]).max() < POSE_TOL
        assert np.abs(m.transform("bef") - g[f"post_bef_{t}"]).max() < 1e-6
        assert np.abs(full - g[f"post_full_{t}"]).max() < 2e-5
        st = m.stats()
        assert [st["iterations"], st["corner_ds"], st["surf_ds"]] == [int(g[f"post_stats_{t}"][0]), int(g[f"post_stats_{t}"][2]), int(g[f"post_stats_{t}"][3])]
        # the map after the step, point for point: the fixture only stores the sizes, so the oracle takes the same step from the
        # same stored state (tests/test_ref_pinning.py: it reproduces the fixture, as does the reference's own code)
        o = op.LaserMapping(orc)
        o.load_cubes(g[f"pre_corner_cubes_{t}"], g[f"pre_surf_cubes_{t}"])
        o.set_transform("aft", g[f"pre_aft_{t}"])
        o.set_transform("bef", g[f"pre_bef_{t}"])
        o.set_inputs(g[f"corner_last_{t}"], g[f"surf_last_{t}"], g[f"full_{t}"], g[f"sum_{t}"])
        assert o.process()
        assert len(o.cloud("corner_cubes")) == int(g[f"post_n_corner_{t}"]) and len(o.cloud("surf_cubes")) == int(g[f"post_n_surf_{t}"])
        _assert_same_point_set(m.cubes("corner"), o.cloud("corner_cubes"), (t, "corner_cubes"))
        _assert_same_point_set(m.cubes("surf"), o.cloud("surf_cubes"), (t, "surf_cubes"))


def test_free_running_slam(orc, small_world):
    """8 sweeps without re-synchronisation: both sides track the ground truth; their mutual drift stays bounded."""
    n = 8
    poses = synth.trajectory(n)
    osr, ood, omp, g = op.ScanRegistration(orc), op.LaserOdometry(orc), op.LaserMapping(orc), loamx.LaserMapping()
    drift = 0.0
    for k in range(n):
        sw = synth.make_sweep(small_world, "VLP-16", poses[k], poses[k + 1], seed=k, az_steps=1200)
        ood.set_features(osr.process(sw.points, sw.ring_sizes))
        ood.process()
        full_end, lc, ls, ts = ood.full_to_end(), ood.last_corner(), ood.last_surf(), ood.transform_sum
        omp.set_inputs(lc, ls, full_end, ts)
        omp.process()
        g.update_odometry(ts)
        g.process(lc, ls, full_end)
        drift = max(drift, float(np.abs(omp.transform("aft") - g.transform("aft")).max()))
        assert omp.has_fresh_map() == g.has_fresh_map()
        if g.has_fresh_map():
            so, sg = omp.cloud("surround_ds"), g.surround()
            assert abs(len(so) - len(sg)) <= max(4, len(so) // 500)
    aft = g.transform("aft")
    assert np.abs(aft[3:] - poses[n, 3:]).max() < 0.12 and np.abs(aft[:3] - poses[n, :3]).max() < 0.01
    assert drift < 2e-3, drift


def test_first_frames_and_window_shift(orc):
    """Sparse-map early return keeps Bef/Aft stale (:628-629); a pose far from the origin shifts the cube window."""
    rng = np.random.default_rng(1)

    def cloud(n, centre):
        p = np.zeros((n, 4), np.float32)
        p[:, :3] = rng.uniform(-20, 20, (n, 3)) + centre
        return p
    for centre in (np.zeros(3), np.array([420.0, 0.0, -390.0])):     # the second one is 8 cubes from the origin
        omp, g = op.LaserMapping(orc), loamx.LaserMapping()
        ts = np.array([0, 0, 0, centre[0], centre[1], centre[2]], np.float32)
        for k in range(2):
            lc, ls = cloud(40, 0), cloud(600, 0)
            omp.set_inputs(lc, ls, lc, ts)
            omp.process()
            g.update_odometry(ts)
            g.process(lc, ls, lc)
            assert np.abs(omp.transform("aft") - g.transform("aft")).max() < POSE_TOL
            assert np.abs(omp.transform("tobe") - g.transform("tobe")).max() < POSE_TOL
            assert len(omp.cloud("corner_cubes")) == len(g.cubes("corner"))
            assert len(omp.cloud("surf_cubes")) == len(g.cubes("surf"))


def test_imu_blend_in_transform_update(orc, small_world):
    """updateIMU(IMUState2) + laserOdometryTime (mapping side): with an IMU history transformUpdate
    blends 0.2 % of the interpolated IMU roll / pitch into transformTobeMapped BEFORE the new features are inserted and the
    full-resolution cloud is registered (BasicLaserMapping.cpp:171-203).  Per step from an identical prior state."""
    n = 5
    poses = synth.trajectory(n)
    osr, ood, omp = op.ScanRegistration(orc), op.LaserOdometry(orc), op.LaserMapping(orc)
    rng = np.random.default_rng(3)
    imu = [(0.1 * k + 0.0137 * j, 0.02 * np.sin(0.3 * k + j), 0.03 * np.cos(0.2 * k - j)) for k in range(n + 1) for j in range(7)]
    fed = 0
    for k in range(n):
        sw = synth.make_sweep(small_world, "VLP-16", poses[k], poses[k + 1], seed=k, az_steps=900)
        ood.set_features(osr.process(sw.points, sw.ring_sizes))
        ood.process()
        full_end, lc, ls, ts = ood.full_to_end(), ood.last_corner(), ood.last_surf(), ood.transform_sum
        g = loamx.LaserMapping()
        pre_c, pre_s, pre_aft, pre_bef = omp.cloud("corner_cubes"), omp.cloud("surf_cubes"), omp.transform("aft"), omp.transform("bef")
        g.load_cubes(pre_c, pre_s)
        g.set_transform("aft", pre_aft)
        g.set_transform("bef", pre_bef)
        g.update_odometry(ts)
        t_odo = 0.1 * k + 0.033            # between IMU samples: exercises the interpolation branch
        new = [m for m in imu if m[0] <= t_odo + 0.15]
        for m in new[fed:]:
            omp.update_imu(*m)
        for m in new:                      # the fresh GPU handle gets the whole history so far
            g.update_imu(*m)
        fed = len(new)
        omp.set_time(t_odo)
        g.set_time(t_odo)
        omp.set_inputs(lc, ls, full_end, ts)
        assert omp.process()
        rc, gfull = g.process(lc, ls, full_end)
        assert rc == loamx.OK
        for which in ("aft", "bef", "tobe"):
            assert np.abs(omp.transform(which) - g.transform(which)).max() < POSE_TOL, (k, which)
        assert np.abs(omp.cloud("full_res") - gfull).max() < 2e-5   # (poses agree to ~2e-7; points are up to 45 m away)
        # the blend really happened: the same step from the same state without IMU data ends 0.2 % of the way elsewhere
        g2 = loamx.LaserMapping()
        g2.load_cubes(pre_c, pre_s)
        g2.set_transform("aft", pre_aft)
        g2.set_transform("bef", pre_bef)
        g2.update_odometry(ts)
        g2.process(lc, ls, full_end)
        plain, blended = g2.transform("tobe"), g.transform("tobe")
        if g.stats()["optimized"]:
            pitch_i = (blended[0] - 0.998 * plain[0]) / 0.002      # the IMU pitch the blend must have used
            roll_i = (blended[2] - 0.998 * plain[2]) / 0.002
            assert abs(pitch_i) < 0.035 and abs(roll_i) < 0.035 and abs(blended[0] - plain[0]) > 1e-7
            assert np.abs(blended[[1, 3, 4, 5]] - plain[[1, 3, 4, 5]]).max() < 1e-6


def test_snapshot_restore_continues_bit_for_bit(orc, small_world, tmp_path):
    """a map snapshot on disk; the restored handle continues exactly like the one that wrote it"""
    n = 7
    poses = synth.trajectory(n)
    osr, ood = op.ScanRegistration(orc), op.LaserOdometry(orc)
    g = loamx.LaserMapping()
    steps = []
    for k in range(n):
        sw = synth.make_sweep(small_world, "VLP-16", poses[k], poses[k + 1], seed=k, az_steps=900)
        ood.set_features(osr.process(sw.points, sw.ring_sizes))
        ood.process()
        steps.append((ood.last_corner(), ood.last_surf(), ood.full_to_end(), ood.transform_sum))
    path = str(tmp_path / "map.loamx")
    for k in range(4):
        g.update_odometry(steps[k][3])
        g.process(*steps[k][:3])
    g.save_snapshot(path)
    assert os.path.getsize(path) > 16 * (len(g.cubes("corner")) + len(g.cubes("surf")))
    r = loamx.LaserMapping()
    r.load_snapshot(path)
    for which in ("corner", "surf"):
        assert np.array_equal(g.cubes(which), r.cubes(which))
    for k in range(4, n):
        outs = []
        for h in (g, r):
            h.update_odometry(steps[k][3])
            rc, full = h.process(*steps[k][:3])
            outs.append((rc, full, h.transform("aft"), h.transform("bef"), h.has_fresh_map(), h.cubes("corner"), h.cubes("surf"),
                         h.surround() if h.has_fresh_map() else None))
        a, b = outs
        assert a[0] == b[0] and a[4] == b[4]
        for i in (1, 2, 3, 5, 6):
            assert np.array_equal(a[i], b[i]), (k, i)
        if a[4]:
            assert np.array_equal(a[7], b[7])
    with pytest.raises(loamx.LoamxError):
        loamx.LaserMapping(corner_filter_size=0.3).load_snapshot(path)          # other map filter sizes
    with pytest.raises(loamx.LoamxError):
        r.load_snapshot(str(tmp_path / "missing.loamx"))


def test_epoch_merge_insert_equals_the_map_side_of_process(orc, small_world):
    """loamx_map_insert (the merge step of a map epoch): a sweep registered ELSEWHERE — here by the oracle's process(), in
    production by the batched pipeline against a frozen copy of the map — is inserted with its final pose into a map that starts from
    the same cubes.  What comes out must be the map the oracle's own process() leaves behind (BasicLaserMapping.cpp:512-593: stack,
    down-size, insert, re-filter the touched cubes): the same point sets.  The one difference by construction: the stack's round trip
    through the map frame (:279-292, :512-520) uses the final pose instead of the guess — a rounding-level change of the points that are
    averaged (tolerance 5e-5 m at up to 45 m range, a few voxel-face flips)."""
    n = 6
    poses = synth.trajectory(n)
    osr, ood, omp = op.ScanRegistration(orc), op.LaserOdometry(orc), op.LaserMapping(orc)
    acc = loamx.LaserMapping()          # the epoch's accumulator: follows the oracle's map through inserts alone
    worst, grew = 0.0, 0
    for k in range(n):
        sw = synth.make_sweep(small_world, "VLP-16", poses[k], poses[k + 1], seed=40 + k, az_steps=1200)
        ood.set_features(osr.process(sw.points, sw.ring_sizes))
        ood.process()
        lc, ls = ood.last_corner(), ood.last_surf()
        if k == 0:
            acc.load_cubes(omp.cloud("corner_cubes"), omp.cloud("surf_cubes"))
        before = len(acc.cubes("corner")) + len(acc.cubes("surf"))
        omp.set_inputs(lc, ls, ood.full_to_end(), ood.transform_sum)
        assert omp.process()
        assert acc.insert(lc, ls, omp.transform("aft")) == loamx.OK
        for name, which in (("corner_cubes", "corner"), ("surf_cubes", "surf")):
            worst = max(worst, _assert_same_point_set(acc.cubes(which), omp.cloud(name), (k, name), tol=5e-5, max_flips=8))
        grew += int(len(acc.cubes("corner")) + len(acc.cubes("surf")) > before)
        assert acc.stats()["iterations"] == 0          # nothing was optimised
    assert grew >= n - 1
    # a handle that went through process() itself holds the same map as the one that was only told the poses
    print(f"epoch merge: worst matched map-point distance {worst:.2e} over {n} inserts")


def test_full_res_registered_when_a_sweep_converges_after_the_first_look(orc, small_world):
    """One handle, two sweeps.  Sweep 1 starts from its true pose and converges at once, so the registration's first chunk for sweep 2
    is max(it1 + 1, 2) launches (csrc/reg_schedule.hpp); sweep 2 starts 1 m off and needs more than that but fewer than the bound: it
    converges at a LATER look, behind the speculative full-resolution launch, which passed it over.  Its cloud must still come back in
    the map frame (the closing mode-2 launch); left out, the points stay in the sensor frame, off by the whole pose.  The displacement
    was chosen with the oracle, whose counts for it are it1 = 1, it2 = 5."""
    n = 5
    poses = synth.trajectory(n)
    osr, ood, omp = op.ScanRegistration(orc), op.LaserOdometry(orc), op.LaserMapping(orc)
    steps = []
    for k in range(n):
        sw = synth.make_sweep(small_world, "VLP-16", poses[k], poses[k + 1], seed=k, az_steps=1200)
        ood.set_features(osr.process(sw.points, sw.ring_sizes))
        ood.process()
        cubes = (omp.cloud("corner_cubes"), omp.cloud("surf_cubes"))
        inputs = (ood.last_corner(), ood.last_surf(), ood.full_to_end(), ood.transform_sum)
        omp.set_inputs(*inputs)
        assert omp.process()
        steps.append((cubes, inputs, omp.transform("aft")))
    displacement = np.array([0.0, 0.05, 0.0, 1.0, 0.0, 0.6], np.float32)
    max_iterations = 10
    o, g = op.LaserMapping(orc), loamx.LaserMapping()
    o.load_cubes(*steps[3][0])
    g.load_cubes(*steps[3][0])
    iters, full = {}, None
    for k, off in ((3, 0 * displacement), (4, displacement)):
        _, (lc, ls, full_end, ts), true_pose = steps[k]
        for h in (o, g):                       # the guess is aft o (bef^-1 o sum): with bef = sum it is aft itself
            h.set_transform("aft", true_pose + off)
            h.set_transform("bef", ts)
        o.set_inputs(lc, ls, full_end, ts)
        assert o.process()
        g.update_odometry(ts)
        rc, full = g.process(lc, ls, full_end)
        assert rc == loamx.OK
        iters[k] = (o.stats()["iterations"], g.stats()["iterations"])
    print(f"iterations (oracle, device): sweep 1 {iters[3]}, sweep 2 {iters[4]}")
    for side in (0, 1):
        it1, it2 = iters[3][side], iters[4][side]
        assert max(it1 + 1, 2) < it2 < max_iterations, (side, it1, it2)
    # the input cloud under the returned pose (rotateZXY + translation, BasicLaserMapping.cpp:282-292), in double
    rx, ry, rz, tx, ty, tz = (float(v) for v in g.transform("aft"))
    x, y, z = steps[4][1][2][:, :3].astype(np.float64).T
    x, y = np.cos(rz) * x - np.sin(rz) * y, np.sin(rz) * x + np.cos(rz) * y
    y, z = np.cos(rx) * y - np.sin(rx) * z, np.sin(rx) * y + np.cos(rx) * z
    x, z = np.cos(ry) * x + np.sin(ry) * z, np.cos(ry) * z - np.sin(ry) * x
    want = np.stack([x + tx, y + ty, z + tz], 1)
    assert len(full) == len(want)
    d = float(np.abs(full[:, :3] - want).max())
    print(f"registered full-resolution cloud of sweep 2 against the input under the returned pose: {d:.2e}")
    assert d < 2e-5, d   # (as the other full-resolution comparisons of this scene; the oracle's own cloud is 9e-6 from the double product)
    assert np.abs(g.transform("aft") - o.transform("aft")).max() < POSE_TOL
