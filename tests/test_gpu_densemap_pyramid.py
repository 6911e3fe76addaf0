"""GPU: the dense map's coarser levels and the coarse-to-fine alignment (loamx_densemap_coarsen, loamx_densemap_freeze_pyramid,
loamx_densemap_align_select_level, loamx_densemap_align_pyramid) against their model (tests/densemap_pyramid_model.py).

coarsen: every key and every one of the thirteen words per voxel equal to the model's cascade fed the model map's words, and, on dyadic
points, to what a handle of the coarser leaf holds.  A level's step: the snapshot the model sees is the level's words from coarsen
through loamx_densemap_surfel_of at the level's leaf (the entries a freeze_pyramid keeps, by definition), so all 28 sums and 5 counts
are compared integer for integer.  align_pyramid: byte for byte the chain select_level + align.  The basin case: the bars of
tests/test_gpu_densemap_align.py's loop test (0.01 rad, leaf / 10, 4 x the model's own error) from a start the single loop cannot use."""
import numpy as np
import pytest

import densemap_align_model as am
import densemap_carve_model as cm
import densemap_model as dm
import densemap_moments_model as mm
import densemap_pyramid_model as pm
from loam_velodyne_amd import loamx
from test_gpu_densemap_carve import mover_calls

pytestmark = pytest.mark.gpu

LEAF = pm.BASIN_LEAF


def _pair(leaf=LEAF, carving=False):
    d = loamx.DenseMap(leaf=leaf, initial_slots=1024)
    if carving:
        d.enable_carving()
    d.enable_moments()
    return d, (mm.CarveMomentsModel(leaf=leaf) if carving else mm.MomentsModel(leaf=leaf))


def _feed(d, m, calls):
    for p, o in calls:
        assert d.add(p, o) == loamx.OK
        assert m.add(p, o)


def _check_coarsen(d, m, static=None, keep=None, levels=3):
    """levels 1 .. `levels` of the device against the model's cascade, word for word; returns the device's levels"""
    want = pm.cascade(m.keys, m.vals, m.moments(), levels, keep)
    got = []
    for l in range(1, levels + 1):
        keys, vals, mom = d.coarsen(l, static)
        wk, wv, wm = want[l - 1]
        assert keys.tolist() == wk.tolist(), l
        assert vals.tolist() == wv.tolist(), l
        assert mom.tolist() == wm.tolist(), l
        got.append((keys, vals, mom))
    return got


def test_coarsen_the_dyadic_cloud_and_a_coarser_handle():
    pts = pm.dyadic_cloud()
    d, m = _pair(pm.DYADIC_LEAF)
    _feed(d, m, [(pts, pm.DYADIC_ORIGIN)])
    assert d.rehashes >= 1 and len(m) > 2048    # the source table grew while it was filled
    got = _check_coarsen(d, m)
    for l, (keys, vals, mom) in enumerate(got, start=1):
        leaf_l = pm.DYADIC_LEAF * 2 ** l
        b, mb = _pair(leaf_l)
        _feed(b, mb, [(pts, pm.DYADIC_ORIGIN)])
        assert keys.tolist() == mb.keys.tolist() and vals.tolist() == mb.vals.tolist()
        assert dm.export(keys, vals, leaf_l).tobytes() == b.points().tobytes()
        assert mom.tobytes() == b.moments().tobytes()


def test_coarsen_the_box_sweeps_whole_and_split():
    S = am.box_scene()
    d, m = _pair()
    _feed(d, m, S["sweeps"])
    assert d.rehashes >= 1
    got = _check_coarsen(d, m)
    assert len(got[0][0]) > 256 and len(got[2][0]) > 16
    # the same points split into calls differently (each part with its sweep's origin), into a table that never grows
    big = loamx.DenseMap(leaf=LEAF, initial_slots=1 << 14)
    big.enable_moments()
    for p, o in S["sweeps"]:
        for part in (p[:1], p[1:1500], p[1500:1501], p[1501:]):
            assert big.add(part, o) == loamx.OK
    assert big.rehashes == 0
    for l in (1, 2, 3):
        for a, b in zip(big.coarsen(l), got[l - 1]):
            assert a.tobytes() == b.tobytes()
    # the live table is only read
    assert d.moments().tolist() == m.moments().tolist() and len(d) == len(m)


def test_coarsen_hand_made_voxels():
    rng = np.random.default_rng(12)
    cells = [(x, y, z) for x in (-2, -1, 0, 1) for y in (-2, -1, 0, 1) for z in (-2, -1, 0, 1)]    # eight parents with all eight children
    cells += [(11, 10, 9)]                                  # a parent with a single child
    cells += [(-((1 << 20) - 1), 3, -((1 << 20) - 1))]      # the lowest index a key holds
    pts = []
    for c in cells:
        u = rng.integers(1, 8, (3, 3)) / 8.0    # offsets on eighths: exact in f32 next to 2^18
        pts.append((np.array(c, np.float64) + u) * LEAF)
    p = np.zeros((3 * len(cells), 4), np.float32)
    p[:, :3] = np.concatenate(pts)
    d, m = _pair()
    _feed(d, m, [(p, (0.5, 0.5, 0.5))])
    assert sorted(m.keys.tolist()) == sorted(pm.key_of(c) for c in cells) and d.rehashes == 0
    got = _check_coarsen(d, m)
    keys1, vals1, _ = got[0]
    assert len(keys1) == 10
    at = {tuple(pm.indices_of(k)): int(n) for k, n in zip(keys1.tolist(), vals1[:, 0].tolist())}
    assert at[(-1, -1, -1)] == 24 and at[(0, 0, 0)] == 24 and at[(5, 5, 4)] == 3 and at[(-(1 << 19), 1, -(1 << 19))] == 3
    assert int(vals1[:, 1:].max()) < 24 << 20
    # an empty map has empty levels
    e, _ = _pair()
    for l in (1, 5):
        assert all(len(a) == 0 for a in e.coarsen(l))


def test_coarsen_leaves_out_the_dynamic_voxels():
    calls, wall, cluster, o = mover_calls()
    rule = loamx.StaticRule()
    d, m = _pair(0.5, carving=True)
    _feed(d, m, [(p, o) for p in calls])
    dyn = m.dynamic_mask(cm.DEFAULT_RULE)
    assert dyn.sum() >= 1 and d.misses().tolist() == m.misses().tolist()
    with_rule = _check_coarsen(d, m, static=rule, keep=~dyn)
    without = _check_coarsen(d, m)
    gone = int(m.vals[dyn, 0].sum())
    for l in range(3):
        assert int(without[l][1][:, 0].sum()) - int(with_rule[l][1][:, 0].sum()) == gone > 0


def _level_tables(d, m, levels, max_curvature=0.0):
    """[(keys, records)] of the snapshots of a pyramid as the model takes them: level 0 from surfels() under the model map's keys,
    level l from coarsen(l) through loamx_densemap_surfel_of at the level's leaf"""
    tables = [am.frozen_of(m.keys, d.surfels())]
    for l in range(1, levels):
        keys, vals, mom = d.coarsen(l)
        leaf_l = d.level_leaf(l)
        surf = np.array([loamx.surfel_of(leaf_l, pm.indices_of(k), v, w) for k, v, w in zip(keys.tolist(), vals.tolist(), mom.tolist())],
                        np.float32).reshape(-1, 8)
        tables.append(pm.frozen_of_level(keys, surf, max_curvature))
    return tables


@pytest.fixture(scope="module")
def box():
    S = am.box_scene()
    d, m = _pair()
    _feed(d, m, S["sweeps"])
    S["map"], S["model"] = d, m
    S["n"] = d.freeze_pyramid(levels=3)
    S["tables"] = _level_tables(d, m, 3)
    assert S["n"] == [len(t[0]) for t in S["tables"]] and d.frozen_levels == 3
    return S


def test_level_0_is_freeze(box):
    S = box
    a, ma = _pair()
    _feed(a, ma, S["sweeps"])
    n = a.freeze()
    b = S["map"]
    b.select_level(0)
    assert n == a.frozen_size == b.frozen_size == S["n"][0] and a.frozen_levels == 1 and b.frozen_levels == 3
    P = S["start"]
    rtc = am.rtc_of(P[:, :3], P[:, 3])
    for nb in (0, 1):
        sa, ca = a.align_step(S["cloud"], rtc, nb)
        sb, cb = b.align_step(S["cloud"], rtc, nb)
        assert sa.tobytes() == sb.tobytes() and ca.tobytes() == cb.tobytes() and int(ca[am.MATCHED]) > 500
    ra, rb = a.align(S["cloud"], P), b.align(S["cloud"], P)
    assert ra["pose"].tobytes() == rb["pose"].tobytes() and {k: v for k, v in ra.items() if k != "pose"} == {k: v for k, v in rb.items() if k != "pose"}
    # a plain freeze drops the coarse levels, a pyramid of one level is a plain freeze
    c, mc = _pair()
    _feed(c, mc, S["sweeps"])
    assert c.frozen_levels == 0
    assert c.freeze_pyramid(levels=2) == S["n"][:2] and c.frozen_levels == 2
    c.select_level(1)
    assert c.freeze() == n and c.frozen_levels == 1
    assert c.align_step(S["cloud"], rtc, 1)[0].tobytes() == sb.tobytes()    # the selection went back to level 0
    assert c.freeze_pyramid(levels=1) == [n] and c.frozen_levels == 1
    c.reset()
    assert c.frozen_levels == 0


@pytest.mark.parametrize("max_curvature", [0.0, 0.02])
def test_a_levels_step_equals_the_model(box, max_curvature):
    S = box
    d, m = _pair()
    _feed(d, m, S["sweeps"])
    n = d.freeze_pyramid(levels=3, max_curvature=max_curvature)
    tables = _level_tables(d, m, 3, max_curvature)
    assert n == [len(t[0]) for t in tables]
    if max_curvature:
        assert n[0] == S["n"][0] and n[1] < S["n"][1] and n[2] < S["n"][2] and n[2] > 10    # corners left out; level 0 is not filtered
    P = S["start"]
    rtcs = np.stack([am.rtc_of(P[:, :3], P[:, 3]), am.rtc_of(S["truth"][:, :3], S["truth"][:, 3]), am.rtc_of()])
    cloud = S["cloud"][:2001]
    stats = d.align_stats()
    for l in (1, 2):
        d.select_level(l)
        leaf_l = d.level_leaf(l)
        keys, recs = tables[l]
        for nb in (0, 1):
            sums, counts = d.align_step(cloud, rtcs[0], nb)
            want_sums, want_counts = am.step(keys, recs, cloud, rtcs[0], leaf_l, nb)
            assert counts.tolist() == want_counts.tolist() and sums.tolist() == want_sums.tolist()
            assert int(counts.sum()) == len(cloud) and counts[am.MATCHED] > 200
            sums_m, counts_m = d.align_step_many(cloud, rtcs, nb)
            for k in range(3):
                w_sums, w_counts = am.step(keys, recs, cloud, rtcs[k], leaf_l, nb)
                assert counts_m[k].tolist() == w_counts.tolist() and sums_m[k].tolist() == w_sums.tolist()
    after = d.align_stats()    # the counters sum over the levels
    assert after["launches"] - stats["launches"] == 8 and after["pose_steps"] - stats["pose_steps"] == 4 + 4 * 3


def _same(a, b):
    return a["pose"].tobytes() == b["pose"].tobytes() and all(a[k] == b[k] for k in ("iterations", "degenerate_dims", "status", "rms", "counts"))


def test_align_pyramid_is_the_composition(box):
    S, d = box, box["map"]
    start = pm.basin_start(S["truth"])
    rtc = am.rtc_of(S["start"][:, :3], S["start"][:, 3])
    cases = ((S["cloud"], start, None, {}), (S["cloud"][:1500], S["start"], np.float32([0.5, -0.25, 1.0]), dict(max_iterations=6, neighbourhood=0)),
             (S["cloud"][:700], start, None, dict(min_matched=701)))
    for first in (2, 1, 0):
        for cloud, pose, centre, cfg in cases:
            d.select_level(1)
            words = d.align_step(cloud, rtc, 1)[0]
            out = d.align_pyramid(cloud, pose, centre, first_level=first, **cfg)
            assert len(out) == first + 1
            assert d.align_step(cloud, rtc, 1)[0].tobytes() == words.tobytes()    # the selected level is still 1
            p = pose
            for k, l in enumerate(range(first, -1, -1)):
                d.select_level(l)
                r = d.align(cloud, p, centre, **cfg)
                assert _same(out[k], r), (first, l)
                p = r["pose"]
            if "min_matched" in cfg:    # every level matched too little and handed its input on
                assert all(o["status"] == 2 and o["iterations"] == 1 and o["pose"].tobytes() == pose.tobytes() for o in out)
    d.select_level(0)
    assert d.align_pyramid(S["cloud"], start)[-1]["pose"].tobytes() == d.align_pyramid(S["cloud"], start, first_level=2)[-1]["pose"].tobytes()


def test_the_basin_case(box):
    """Measured on an MI355X: the figures this prints are recorded in CHANGELOG.md; asserted are the bars against ground truth and the
    margin over the model."""
    S, d = box, box["map"]
    truth = S["truth"]
    start = pm.basin_start(truth)
    out = d.align_pyramid(S["cloud"], start, first_level=2)
    want = pm.align_pyramid(S["tables"], S["cloud"], start, LEAF)
    rot, trans = am.pose_error(out[-1]["pose"], truth)
    rot_m, trans_m = am.pose_error(want[-1]["pose"], truth)
    d_rot, d_trans = am.pose_error(out[-1]["pose"], want[-1]["pose"])
    d.select_level(0)
    single = d.align(S["cloud"], start)
    rot_s, trans_s = am.pose_error(single["pose"], truth)
    print(f"pyramid: library iterations {[o['iterations'] for o in out]}, status {[o['status'] for o in out]}, {rot:.3e} rad, {trans:.3e} m, "
          f"rms {out[-1]['rms']:.5f}; model iterations {[w['iterations'] for w in want]}, {rot_m:.3e} rad, {trans_m:.3e} m, "
          f"rms {want[-1]['rms']:.5f}; library against model {d_rot:.3e} rad, {d_trans:.3e} m; "
          f"single level: status {single['status']}, {single['iterations']} iterations, {rot_s:.3e} rad, {trans_s:.3e} m")
    assert rot <= 0.01 and trans <= LEAF / 10
    assert rot <= 4.0 * rot_m and trans <= 4.0 * trans_m
    assert trans_s > LEAF


def test_invalid_arguments(box):
    S, d = box, box["map"]
    d.select_level(2)
    rtc = am.rtc_of(S["start"][:, :3], S["start"][:, 3])
    words = d.align_step(S["cloud"][:500], rtc, 1)[0]
    plain = loamx.DenseMap(leaf=LEAF, initial_slots=1024)    # moments off
    plain.add(S["sweeps"][0][0], S["sweeps"][0][1])
    refused = [lambda: d.freeze_pyramid(levels=0), lambda: d.freeze_pyramid(levels=7), lambda: d.freeze_pyramid(max_curvature=-0.1),
               lambda: d.freeze_pyramid(max_curvature=float("nan")), lambda: d.coarsen(0), lambda: d.coarsen(6), lambda: d.select_level(3),
               lambda: plain.coarsen(1), lambda: plain.freeze_pyramid(), lambda: d.coarsen(1, loamx.StaticRule()),
               lambda: d.freeze_pyramid(static=loamx.StaticRule()), lambda: d.align_pyramid(S["cloud"], S["start"], first_level=3),
               lambda: d.align_pyramid(S["cloud"], S["start"], first_level=2, neighbourhood=2),
               lambda: d.align_pyramid(S["cloud"], np.full((3, 4), np.inf), first_level=1), lambda: plain.select_level(0),
               lambda: plain.align_pyramid(S["cloud"], S["start"], first_level=0)]
    for k, call in enumerate(refused):
        with pytest.raises(loamx.LoamxError) as e:
            call()
        assert e.value.code == loamx.E_INVALID, k
    # the handle is as it was: three levels, level 2 selected, the same words
    assert d.frozen_levels == 3 and d.frozen_size == S["n"][0] and plain.frozen_levels == 0
    assert d.align_step(S["cloud"][:500], rtc, 1)[0].tobytes() == words.tobytes()
    d.select_level(0)
