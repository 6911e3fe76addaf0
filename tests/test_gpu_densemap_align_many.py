"""GPU: alignment from many start poses at once (loamx_densemap_align_step_many, loamx_densemap_align_many and its from_* forms) against
the oracle that is already in the tree: K calls of the single-pose functions, word for word and byte for byte, and for the steps the
numpy model (tests/densemap_align_model.py) integer for integer.  Nothing here has a tolerance except the recovery of the wide start,
whose bars are those of the single alignment's tests: 0.01 rad and leaf / 10 against ground truth.

The maps are built through the library as in tests/test_gpu_densemap_align.py (its small helpers are copied, not imported)."""
import ctypes as C

import numpy as np
import pytest

import densemap_align_model as am
import densemap_model as dm
from loam_velodyne_amd import loamx, synth

pytestmark = pytest.mark.gpu

LEAF = 0.5
NONE = 0xFFFFFFFF


def _map_of(sweeps, leaf=LEAF, carving=False, **freeze):
    """(device map with moments, frozen; keys, records of the snapshot as the model takes them)"""
    d = loamx.DenseMap(leaf=leaf, initial_slots=1024)
    if carving:
        d.enable_carving()
    d.enable_moments()
    m = dm.Model(leaf=leaf)
    for p, o in sweeps:
        assert d.add(p, o) == loamx.OK
        assert m.add(p, o)
    n = d.freeze(**freeze)
    keys, recs = am.frozen_of(m.keys, d.surfels(**freeze))
    assert n == len(keys) == d.frozen_size
    return d, keys, recs


@pytest.fixture(scope="module")
def box():
    S = am.box_scene()
    S["map"], S["keys"], S["recs"] = _map_of(S["sweeps"], S["leaf"])
    assert 400 < len(S["keys"]) <= 512
    return S


@pytest.fixture(scope="module")
def plane():
    d, keys, recs = _map_of([(am.lattice_plane(), am.PLANE_ORIGIN)])
    assert len(keys) == 256 and np.all(recs[:, 3:] == np.float32([0, 0, 1]))
    return dict(map=d, keys=keys, recs=recs, cloud=am.lattice_plane()[::3].copy())


def _mixed_cloud(S, n):
    """n points for steps in the box: scene points, the first half in the map frame (for the identity), the second in the sensor frame
    (for the general start), with the special cases of the single step's test in front, as far as n has room for them"""
    rng = np.random.default_rng(2000 + n)
    p = am.box_points(rng, n, sigma=0.05)
    P = S["truth"]
    h = n // 2
    p[h:, :3] = (p[h:, :3].astype(np.float64) - P[:, 3]) @ P[:, :3]
    on_face = am.box_points(rng, 6)[:, :3]
    on_face[:3] = np.round(on_face[:3] * 2.0) / 2.0            # on a cell corner
    on_face[3:, 0] = np.round(on_face[3:, 0] * 2.0) / 2.0      # on a face across x
    special = [np.float32([np.nan, 0.0, 0.0]), np.float32([1500.0, 0.0, 0.0]), np.float32([0.0, -1024.0, 0.0]),   # far
               np.float32([0.0, 0.0, 1000.0]),                                                                     # near, unmatched
               np.float32([0.2, 0.1, 0.3]), np.float32([-2.2, 0.1, 0.3])] + [f for f in on_face]                   # mid-air, 0.7 m off a wall
    for k, s in enumerate(special[:max(n - 1, 0)]):
        p[k + 1, :3] = s
    return p


IDENTITY, GENERAL, TWIN, ALL_FAR, ALL_OUTSIDE, ALL_UNMATCHED = range(6)


def _pose_pool(S, K):
    """K step poses (K, 15): the identity, the scene's general start, the same again, one whose centre throws every point FAR (FAR
    tests a = R (p - c), which no translation reaches), one that carries every point OUTSIDE the key range, one 50 m away where nothing
    is matched (whole waves without a match); beyond those, small perturbations of the start"""
    P = S["start"]
    pool = [am.rtc_of(), am.rtc_of(P[:, :3], P[:, 3]), am.rtc_of(P[:, :3], P[:, 3]), am.rtc_of(c=(5000.0, 0.0, 0.0)),
            am.rtc_of(t=(600000.0, 0.0, 0.0)), am.rtc_of(P[:, :3], P[:, 3] + [0.0, 50.0, 0.0])]
    rng = np.random.default_rng(40 + K)
    while len(pool) < K:
        R = am.exp_so3(rng.normal(0.0, 0.03, 3)) @ P[:, :3]
        pool.append(am.rtc_of(R, P[:, 3] + rng.normal(0.0, 0.1, 3)))
    return np.stack(pool[:K])


def _check_many(S, cloud, rtcs, nb, max_residual=None, leaf=LEAF, model=True):
    """align_step_many against K calls of align_step (bytes) and, with model, against the numpy step (integers)"""
    d = S["map"]
    sums, counts = d.align_step_many(cloud, rtcs, nb, max_residual)
    assert sums.shape == (len(rtcs), 28) and counts.shape == (len(rtcs), 5)
    for k, rtc in enumerate(rtcs):
        s1, c1 = d.align_step(cloud, rtc, nb, max_residual)
        assert sums[k].tobytes() == s1.tobytes() and counts[k].tobytes() == c1.tobytes(), k
        if model:
            want_sums, want_counts = am.step(S["keys"], S["recs"], cloud, rtc, leaf, nb, max_residual)
            assert counts[k].tolist() == want_counts.tolist(), (k, counts[k], want_counts)
            assert sums[k].tolist() == want_sums.tolist(), k
    return sums, counts


@pytest.mark.parametrize("nb", [0, 1])
@pytest.mark.parametrize("K", [1, 2, 3, 17])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 5000])
def test_step_many_equals_k_steps_and_the_model(box, n, K, nb):
    cloud = _mixed_cloud(box, n)
    rtcs = _pose_pool(box, K)
    sums, counts = _check_many(box, cloud, rtcs, nb)
    assert np.all(counts.sum(axis=1) == n)
    if K >= 3:
        assert sums[TWIN].tobytes() == sums[GENERAL].tobytes() and counts[TWIN].tobytes() == counts[GENERAL].tobytes()
    if n >= 65:
        for k in range(min(K, 2)):
            assert counts[k, am.FAR] >= 2 and counts[k, am.UNMATCHED] >= 1 and counts[k, am.MATCHED] > n // 8
    if K == 17:
        n_nan = int(np.isnan(cloud[:, 0]).sum())
        assert counts[ALL_FAR].tolist() == [n, 0, 0, 0, 0] and not sums[ALL_FAR].any()
        n_far = int(counts[IDENTITY, am.FAR])    # (the pose is a translation: the FAR points of the identity)
        assert counts[ALL_OUTSIDE].tolist() == [n_far, n - n_far, 0, 0, 0] and n_far >= n_nan
        assert counts[ALL_UNMATCHED, am.MATCHED] == 0 and counts[ALL_UNMATCHED, am.UNMATCHED] >= n - 3 and not sums[ALL_UNMATCHED].any()
        # permuting the poses permutes the outputs and nothing else
        perm = np.random.default_rng(9).permutation(K)
        sums_p, counts_p = box["map"].align_step_many(cloud, rtcs[perm], nb)
        assert sums_p.tobytes() == sums[perm].tobytes() and counts_p.tobytes() == counts[perm].tobytes()
        if n == 5000:
            # a tight bound: REJECTED points
            _, counts_r = _check_many(box, cloud, rtcs, nb, max_residual=0.05)
            assert counts_r[GENERAL, am.REJECTED] > n // 20 and counts_r[GENERAL, am.MATCHED] > n // 20
            # the cloud as PCL records: identical words
            sums_l, counts_l = box["map"].align_step_many(loamx.to_pcl_layout(cloud), rtcs, nb)
            assert sums_l.tobytes() == sums.tobytes() and counts_l.tobytes() == counts.tobytes()


def test_step_many_midpoint_tie(plane):
    # x = 0.4375 is exactly as far from the mean of cell 0 (0.1875) as from that of cell 1 (0.6875); whole-cell translations keep the tie
    p = np.zeros((70, 4), np.float32)
    p[:, 0] = 0.4375 + 0.5 * (np.arange(70) % 7 - 3)
    p[:, 1] = 0.1875 + 0.5 * (np.arange(70) // 7 - 5)
    p[:, 2] = 0.0625
    rtcs = np.stack([am.rtc_of(), am.rtc_of(t=(0.5, 0.0, 0.0)), am.rtc_of(t=(-1.0, 0.5, 0.0))])
    for rtc in rtcs:
        _, _, e, which = am.match(plane["keys"], plane["recs"], p, rtc, LEAF, 1)
        assert np.all(e[:, 0] == np.float32(0.25)) and np.all(which >= 0)
    sums, counts = _check_many(plane, p, rtcs, 1)
    assert np.all(counts[:, am.MATCHED] == 70) and np.all(sums[:, 27] == 70 * int(0.0625 ** 2 * 2 ** 24))


def test_step_many_at_the_edge_of_the_key_range():
    x_edge = float(1 << 19)
    patch = am.lattice_plane(x0=x_edge - 4.0, nx=32)
    d, keys, recs = _map_of([(patch, (x_edge - 2.0, 0.2, 2.0))])
    S = dict(map=d, keys=keys, recs=recs)
    cloud = am.lattice_plane(x0=-4.0, nx=64)[::5].copy()
    cloud[:, 2] = 0.03125
    rtcs = np.stack([am.rtc_of(t=(x_edge - 2.0, 0, 0)), am.rtc_of(t=(x_edge - 0.25, 0, 0)), am.rtc_of(t=(-x_edge + 2.0, 0, 0))])
    for nb in (0, 1):
        sums, counts = _check_many(S, cloud, rtcs, nb)
        assert np.all(counts[:, am.OUTSIDE] > 100) and not counts[:, am.FAR].any()
        assert (counts[:, am.MATCHED] > 100).tolist() == [True, True, False]


def test_step_many_with_a_grown_table():
    rng = np.random.default_rng(77)
    leaf = 0.2
    d, keys, recs = _map_of([(am.box_points(rng, 40_000), (0.4, -0.3, 0.1))], leaf=leaf)
    assert am.table_slots(len(keys)) == 8192
    S = dict(map=d, keys=keys, recs=recs)
    cloud = am.box_points(rng, 5000)
    rtcs = np.stack([am.rtc_of(am.exp_so3(rng.normal(0, 0.02, 3)), rng.normal(0, 0.05, 3)) for _ in range(5)])
    for nb in (0, 1):
        sums, counts = _check_many(S, cloud, rtcs, nb, leaf=leaf)
        assert np.all(counts[:, am.MATCHED] > 2000)


def test_step_many_at_the_largest_pose_count(box):
    K = loamx.ALIGN_MAX_POSES
    cloud = _mixed_cloud(box, 65)
    rng = np.random.default_rng(4096)
    P = box["start"]
    rtcs = np.stack([am.rtc_of(am.exp_so3(w) @ P[:, :3], P[:, 3] + v) for w, v in zip(rng.normal(0, 0.05, (K, 3)), rng.normal(0, 0.2, (K, 3)))])
    rtcs[:6] = _pose_pool(box, 6)
    d = box["map"]
    before = d.align_stats()
    sums, counts = d.align_step_many(cloud, rtcs, 1)
    after = d.align_stats()
    assert [after[k] - before[k] for k in ("launches", "readbacks", "pose_steps")] == [1, 1, K]
    for k in range(K):
        s1, c1 = d.align_step(cloud, rtcs[k], 1)
        assert sums[k].tobytes() == s1.tobytes() and counts[k].tobytes() == c1.tobytes(), k
    assert len(np.unique(sums[:, 27])) > K // 2    # (the poses differ, and so do their words)
    # one pose more is refused, and nothing is written
    L = loamx.lib()
    more = np.concatenate([rtcs, rtcs[:1]])
    s, c = np.full((K + 1, 28), 5, np.int64), np.full((K + 1, 5), 5, np.uint64)
    a = loamx.as_points(cloud)
    cl = loamx.cloud_of(a)
    for n_poses in (K + 1, 0):
        rc = L.loamx_densemap_align_step_many(d.h, C.byref(cl), more.ctypes.data_as(C.c_void_p), C.c_uint32(n_poses), C.c_uint32(1),
                                              C.c_float(0.5), s.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p))
        assert rc == loamx.E_INVALID and "n_poses" in L.loamx_last_error().decode()
    assert np.all(s == 5) and np.all(c == 5)
    assert d.align_stats() == dict(launches=after["launches"] + K, readbacks=after["readbacks"] + K, pose_steps=after["pose_steps"] + K)


# ---- loops --------------------------------------------------------------------------------------------------------------------------
def _align_raw(d, cloud, pose, centre=None, **cfg):
    """loamx_densemap_align, the struct as the library wrote it"""
    a = loamx.as_points(cloud)
    c = loamx.cloud_of(a)
    p = np.ascontiguousarray(pose, np.float64).reshape(12)
    ctr = None if centre is None else np.ascontiguousarray(centre, np.float32)
    k, out = loamx.AlignConfig(**cfg), loamx.AlignResult()
    rc = loamx.lib().loamx_densemap_align(d.h, C.byref(c), p.ctypes.data_as(C.c_void_p), None if ctr is None else ctr.ctypes.data_as(C.c_void_p),
                                          C.byref(k), C.byref(out))
    assert rc == loamx.OK
    return out


def _check_loops(d, cloud, poses, centre=None, **cfg):
    """align_many against align per hypothesis, byte for byte, best against align_best, and the three counters"""
    before = d.align_stats()
    out, best = d.align_many(cloud, poses, centre, raw=True, **cfg)
    after = d.align_stats()
    its = [int(out[k].iterations) for k in range(len(poses))]
    ran = 1 if len(cloud) else 0    # (an empty cloud is read back as zeros without a launch)
    assert [after[k] - before[k] for k in ("launches", "readbacks", "pose_steps")] == [ran * max(its), max(its), ran * sum(its)]
    for k, P in enumerate(poses):
        one = _align_raw(d, cloud, P, centre, **cfg)
        assert bytes(out[k]) == bytes(one), (k, out[k].as_dict(), one.as_dict())
        for f in ("iterations", "degenerate_dims", "status", "rms"):
            assert getattr(out[k], f) == getattr(one, f)
        assert out[k].pose[:] == one.pose[:] and out[k].counts[:] == one.counts[:]
    single = d.align_stats()
    # a single align of I iterations: I, I, I
    assert [single[k] - after[k] for k in ("launches", "readbacks", "pose_steps")] == [ran * sum(its), sum(its), ran * sum(its)]
    assert best == loamx.align_best(out)
    return [out[k].as_dict() for k in range(len(poses))], best


def _far(P, dy=50.0):
    Q = np.array(P, np.float64).copy()
    Q[1, 3] += dy
    return Q


def test_align_many_equals_align_per_hypothesis(box):
    starts = [am.box_scene(case=k)["start"] for k in range(3)]
    # the early enders in front and in the middle, so that the compaction shifts slots
    # (the truth itself is a start that ends within a few iterations, the identity one that is 0.3 rad and 0.6 m off)
    poses = np.stack([_far(starts[0]), starts[0], starts[1], _far(starts[2]), starts[2], box["truth"], np.eye(3, 4)])
    res, best = _check_loops(box["map"], box["cloud"], poses)
    its = [r["iterations"] for r in res]
    print("iterations", its, "status", [r["status"] for r in res], "best", best)
    assert res[0]["status"] == 2 and res[3]["status"] == 2 and its[0] == 1 and its[3] == 1
    assert res[0]["pose"].tobytes() == poses[0].tobytes()
    assert all(res[k]["status"] == 0 for k in (1, 2, 4)) and len(set(its)) >= 3    # hypotheses that end at different iterations
    for k in (1, 2, 4):
        rot, trans = am.pose_error(res[k]["pose"], box["truth"])
        assert rot <= 0.01 and trans <= LEAF / 10
    assert best in (1, 2, 4, 5)
    # cut by max_iterations, as a call of its own with that configuration; neighbourhood 0 too
    res3, _ = _check_loops(box["map"], box["cloud"], poses[[1, 0, 4]], max_iterations=3)
    assert [r["iterations"] for r in res3] == [3, 1, 3] and [r["status"] for r in res3] == [1, 2, 1]
    _check_loops(box["map"], box["cloud"], poses[:5], neighbourhood=0, max_residual=0.3, min_matched=10)
    # one hypothesis alone, and an empty cloud
    _check_loops(box["map"], box["cloud"], poses[1:2])
    res0, best0 = _check_loops(box["map"], box["cloud"][:0], poses[:2])
    assert [r["status"] for r in res0] == [2, 2] and best0 is None


def test_align_many_about_a_centre(box):
    c = np.float32([2.0, -1.0, 0.5])
    poses = []
    for case in (1, 2):
        start = am.box_scene(case=case)["start"].copy()
        start[:, 3] -= start[:, :3] @ c.astype(np.float64)
        poses.append(start)
    cloud = box["cloud"].copy()
    cloud[:, :3] += c
    truth = box["truth"].copy()
    truth[:, 3] -= truth[:, :3] @ c.astype(np.float64)
    res, best = _check_loops(box["map"], cloud, np.stack(poses + [_far(poses[0])]), centre=c)
    for r in res[:2]:
        rot, trans = am.pose_error(r["pose"], truth)
        assert r["status"] == 0 and rot <= 0.01 and trans <= LEAF / 10
    assert res[2]["status"] == 2 and best in (0, 1)


def test_align_many_on_the_exact_plane(plane):
    P = np.concatenate([am.exp_so3([0.01, -0.02, 0.0]), np.array([[0.05], [-0.03], [0.04]])], axis=1)
    Q = np.concatenate([am.exp_so3([-0.015, 0.01, 0.0]), np.array([[-0.07], [0.11], [-0.05]])], axis=1)
    far = np.concatenate([am.exp_so3([0.01, 0.0, 0.02]), np.array([[0.3], [0.1], [50.0]])], axis=1)
    res, best = _check_loops(plane["map"], plane["cloud"], np.stack([P, far, Q]))
    for r, start in ((res[0], P), (res[2], Q)):
        assert r["status"] == 0 and r["degenerate_dims"] == 3 and r["iterations"] <= 4
        assert r["pose"][0, 3] == start[0, 3] and r["pose"][1, 3] == start[1, 3]    # t_x, t_y: not observable, not touched, bit for bit
        assert abs(r["pose"][2, 3]) < 1e-5 and r["rms"] < 1e-5 and r["counts"]["matched"] == len(plane["cloud"])
    assert res[1]["status"] == 2 and res[1]["pose"].tobytes() == far.tobytes() and best in (0, 2)


def test_wide_start_needs_many_starts(box):
    """the start of the issue: 1.1 rad of yaw and (1.5, 0, -1.0) m off.  One alignment ends far from the truth; the best of the 108
    starts of a pose grid (12 yaws of pi / 6, 3 x 3 offsets of 1 m) ends inside the bars.  Asserted is the error of the best start, not
    its index: rms differences of 1e-9 between equally good starts may reorder them"""
    cloud, truth = box["cloud"][::4].copy(), box["truth"]
    wide = loamx.pose_grid(truth, yaws=[1.1], offsets=[(1.5, 0.0, -1.0)])[0]
    single = box["map"].align(cloud, wide)
    rot, trans = am.pose_error(single["pose"], truth)
    print(f"single: status {single['status']}, {rot:.3f} rad, {trans:.3f} m, counts {single['counts']}")
    assert not (rot <= 0.01 and trans <= LEAF / 10)
    grid = loamx.pose_grid(wide, yaws=np.arange(12) * np.pi / 6, offsets=[(dx, 0.0, dz) for dx in (-1.0, 0.0, 1.0) for dz in (-1.0, 0.0, 1.0)])
    assert grid.shape == (108, 3, 4)
    before = box["map"].align_stats()
    res, best = box["map"].align_many(cloud, grid)
    after = box["map"].align_stats()
    assert best is not None
    rot, trans = am.pose_error(res[best]["pose"], truth)
    inside = sum(1 for r in res if (lambda e: e[0] <= 0.01 and e[1] <= LEAF / 10)(am.pose_error(r["pose"], truth)))
    print(f"best of 108: start {best}, {rot:.2e} rad, {trans:.2e} m, rms {res[best]['rms']:.5f}, counts {res[best]['counts']}; {inside} starts "
          f"inside the bars; {after['launches'] - before['launches']} launches for {after['pose_steps'] - before['pose_steps']} pose-steps")
    assert rot <= 0.01 and trans <= LEAF / 10
    assert after["launches"] - before["launches"] == max(r["iterations"] for r in res) <= 20


def test_align_many_from_map():
    w = synth.World(half_extent=65.0)
    cmap, smap = w.make_map(60_000)
    poses = synth.trajectory(1)
    sw = synth.make_sweep(w, "VLP-16", poses[0], poses[1], seed=900, az_steps=900)
    sr, od, mp = loamx.ScanRegistration(), loamx.LaserOdometry(), loamx.LaserMapping()
    mp.load_cubes(cmap, smap)
    d = loamx.DenseMap(leaf=LEAF, initial_slots=1 << 14)
    d.enable_moments()
    with pytest.raises(loamx.LoamxError) as e:
        d.align_many_from(mp)    # nothing frozen yet
    assert e.value.code == loamx.E_INVALID and "nothing is frozen" in str(e.value)
    assert d.freeze() == 0
    rc, _, best = d.align_many_from(mp)
    assert rc == loamx.SKIPPED and best is None    # the mapper has not processed a sweep
    f = sr.process(sw.points.copy(), sw.ring_sizes)
    od.process(f)
    lc, ls = od.last_clouds()
    full = od.transform_to_end(f["full"])
    mp.update_odometry(od.transform_sum)
    mp.process(lc, ls, full)
    assert d.add_from(mp) == loamx.OK
    assert d.freeze() > 50
    shifted = np.eye(3, 4)
    shifted[0, 3] = 0.2
    rc, out, best = d.align_many_from(mp, np.stack([np.eye(3, 4), shifted]), raw=True)
    k, one = loamx.AlignConfig(), loamx.AlignResult()
    assert loamx.lib().loamx_densemap_align_from_map(d.h, mp.h, None, C.byref(k), C.byref(one)) == loamx.OK
    assert rc == loamx.OK and bytes(out[0]) == bytes(one) and one.counts[4] > 1000
    two = loamx.AlignResult()
    assert loamx.lib().loamx_densemap_align_from_map(d.h, mp.h, shifted.ctypes.data_as(C.c_void_p), C.byref(k), C.byref(two)) == loamx.OK
    assert bytes(out[1]) == bytes(two) and best == loamx.align_best(out)
    # poses None: the identity alone
    rc, out1, best1 = d.align_many_from(mp, raw=True)
    assert rc == loamx.OK and bytes(out1[0]) == bytes(one) and best1 == (None if one.status == 2 else 0)
    # NULL poses with more than one pose: refused, nothing written
    out2, b = (loamx.AlignResult * 2)(), C.c_uint32(7)
    assert loamx.lib().loamx_densemap_align_many_from_map(d.h, mp.h, None, C.c_uint32(2), C.byref(k), out2, C.byref(b)) == loamx.E_INVALID
    assert "poses_in" in loamx.lib().loamx_last_error().decode() and b.value == 7 and bytes(out2) == bytes(C.sizeof(out2))


def test_refusals(box):
    d, L = box["map"], loamx.lib()
    cloud = box["cloud"][:100]
    poses = np.stack([box["start"], np.eye(3, 4)])
    stats = d.align_stats()
    for bad, word in ((dict(neighbourhood=2), "neighbourhood"), (dict(max_residual=17.0), "max_residual"), (dict(max_iterations=0), "max_iterations"),
                      (dict(degenerate_ratio=1.0), "degenerate_ratio"), (dict(eps_rot=-1.0), "eps_rot")):
        with pytest.raises(loamx.LoamxError) as e:
            d.align_many(cloud, poses, **bad)
        assert e.value.code == loamx.E_INVALID and word in str(e.value)
    for bad in (dict(neighbourhood=2), dict(max_residual=0.0), dict(max_residual=16.5), dict(max_residual=float("nan"))):
        with pytest.raises(loamx.LoamxError) as e:
            d.align_step_many(cloud, _pose_pool(box, 2), **bad)
        assert e.value.code == loamx.E_INVALID
    # raw calls: nothing is written on a refusal
    a = loamx.as_points(cloud)
    cl = loamx.cloud_of(a)
    k = loamx.AlignConfig()
    nan_pose = poses.copy()
    nan_pose[1, 2, 1] = np.nan    # one bad pose refuses the whole call
    inf_pose = poses.copy()
    inf_pose[0, 0, 3] = np.inf
    big = np.tile(np.eye(3, 4), (loamx.ALIGN_MAX_POSES + 1, 1, 1))
    out, b = (loamx.AlignResult * (loamx.ALIGN_MAX_POSES + 1))(), C.c_uint32(7)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    for args, word in (((d.h, C.byref(cl), ptr(nan_pose), C.c_uint32(2), None, C.byref(k), out, C.byref(b)), "pose"),
                       ((d.h, C.byref(cl), ptr(inf_pose), C.c_uint32(2), None, C.byref(k), out, C.byref(b)), "pose"),
                       ((d.h, C.byref(cl), ptr(big), C.c_uint32(len(big)), None, C.byref(k), out, C.byref(b)), "n_poses"),
                       ((d.h, C.byref(cl), ptr(poses), C.c_uint32(0), None, C.byref(k), out, C.byref(b)), "n_poses"),
                       ((d.h, C.byref(cl), None, C.c_uint32(2), None, C.byref(k), out, C.byref(b)), "poses_in"),
                       ((d.h, None, ptr(poses), C.c_uint32(2), None, C.byref(k), out, C.byref(b)), "points"),
                       ((d.h, C.byref(cl), ptr(poses), C.c_uint32(2), None, C.byref(k), None, C.byref(b)), "out")):
        assert L.loamx_densemap_align_many(*args) == loamx.E_INVALID
        assert word in L.loamx_last_error().decode(), (word, L.loamx_last_error())
    assert b.value == 7 and bytes(out) == bytes(C.sizeof(out))
    assert d.align_stats() == stats    # and nothing ran
    # best may be NULL; cfg NULL: the defaults
    assert L.loamx_densemap_align_many(d.h, C.byref(cl), ptr(poses), C.c_uint32(2), None, None, out, None) == loamx.OK
    assert bytes(out[0]) == bytes(_align_raw(d, cloud, poses[0]))
    # no snapshot
    e = loamx.DenseMap(leaf=LEAF, initial_slots=1024)
    e.enable_moments()
    for call in (lambda: e.align_many(cloud, poses), lambda: e.align_step_many(cloud, _pose_pool(box, 2))):
        with pytest.raises(loamx.LoamxError) as err:
            call()
        assert err.value.code == loamx.E_INVALID and "nothing is frozen" in str(err.value)
    assert e.align_stats() == dict(launches=0, readbacks=0, pose_steps=0)


def test_snapshot_untouched_by_live_map_growth():
    S = am.box_scene()
    d, keys, recs = _map_of(S["sweeps"])
    poses = np.stack([am.box_scene(case=k)["start"] for k in range(3)])
    rtcs = np.stack([am.rtc_of(P[:, :3], P[:, 3]) for P in poses])
    out, best = d.align_many(S["cloud"], poses, raw=True)
    sums, counts = d.align_step_many(S["cloud"], rtcs)
    rng = np.random.default_rng(8)
    rehashes, slots = d.rehashes, d.stats()["slots"]
    for n, o in ((slots // 2, (0.0, 0.0, 0.0)), (1000, (1.0, 0.5, -0.5))):
        clutter = np.zeros((n, 4), np.float32)
        clutter[:, :3] = rng.uniform(-3.0, 3.0, (n, 3))
        d.add(clutter, o)
    assert d.rehashes > rehashes and d.stats()["slots"] > slots
    out2, best2 = d.align_many(S["cloud"], poses, raw=True)
    sums2, counts2 = d.align_step_many(S["cloud"], rtcs)
    assert bytes(out2) == bytes(out) and best2 == best
    assert sums2.tobytes() == sums.tobytes() and counts2.tobytes() == counts.tobytes()
    # the counters run on through a reset; the snapshot does not
    stats = d.align_stats()
    d.reset()
    assert d.align_stats() == stats and stats["launches"] > 0
    with pytest.raises(loamx.LoamxError) as e:
        d.align_many(S["cloud"], poses)
    assert e.value.code == loamx.E_INVALID and "nothing is frozen" in str(e.value)
