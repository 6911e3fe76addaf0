"""GPU: the rolling map's update (csrc/mapping.hip: k_map_split, k_map_insert, k_map_append_filtered, k_map_hist, the surround kernels,
Mapper::make_plan / shift_counts, the speculative partition and the deferred update) against the exact model of
tests/rolling_map_model.py — uint32 words in STORAGE ORDER, every comparison exact.

tests/rolling_map_cases.py builds the cases; tests/test_rolling_map_cases_cpu.py proves on the CPU that each one reaches the path it
claims and that the model equals the oracle (and the reference's own mapping unit) on it.  The insert path runs every case through
load_cubes / insert / cubes; the process path runs one trajectory with speculation hits, a miss and a window shift, with insert()
calls in between, a surround cloud on every fifth processed frame and a snapshot in the middle.

Found by these tests: the statistics of a sweep without a Gauss-Newton update (every insert(), a process() on a sparse sub-map) gave
corner_ds = surf_ds = 0 although the down-sized clouds were inserted; every insert-path case failed on it, split_1 first.

Which case catches which break (scratch builds of csrc/mapping.hip, each run once on an MI355X; a case fails in test_insert_path):
  k_map_append_filtered writes `base + nf - 1 - v`   every case except append_all_empty (which has no filtered output), and both
                                                     trajectory tests
  cube_abs without `c--`                             split_7 ... split_133121, split_all_dropped, split_per_tile, split_corner_empty,
                                                     split_surf_empty, hist_grid_stride, faces_x / y / z, shift_xp / xm / yp / ym / zp / zm,
                                                     shift_several, shift_threshold_on, shift_out_and_back, sequence_growing,
                                                     sequence_lattice: a negative coordinate changes cube
  `>` for `>=` in the shift loop                     split_7 ... split_133121, split_all_dropped, split_per_tile, split_corner_empty,
                                                     split_surf_empty, shift_xp / yp / zp, shift_several, shift_threshold_on,
                                                     shift_out_and_back: the layer that should leave stays
"""
import os

import numpy as np
import pytest

import rolling_map_cases as rc
import rolling_map_model as rm
from loam_velodyne_amd import loamx

pytestmark = pytest.mark.gpu

SIZES = ("corner_from_map", "surf_from_map", "corner_ds", "surf_ds")


def _same_words(where, got, want):
    a, b = np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    assert a.shape == b.shape, f"{where}: {a.shape[0]} points, the model has {b.shape[0]}"
    if not np.array_equal(a, b):
        rows = np.flatnonzero((a != b).any(axis=1))
        r = int(rows[0])
        raise AssertionError(f"{where}: {len(rows)} of {len(a)} rows differ, first at storage position {r}: {got[r]} != {want[r]}")


def _check_map(where, g, want):
    _same_words(f"{where}: corner map", g.cubes("corner"), want["corner"])
    _same_words(f"{where}: surf map", g.cubes("surf"), want["surf"])
    st = g.stats()
    assert {k: st[k] for k in SIZES} == want["stats"], f"{where}: {st}"
    return st


@pytest.mark.parametrize("name", rc.NAMES)
def test_insert_path(orc, name):
    case = rc.get(name)
    loaded, steps = rc.model(orc, name)
    g = loamx.LaserMapping()
    try:
        g.load_cubes(*case.seed)
        _same_words(f"{name}: corner map as loaded", g.cubes("corner"), loaded[0])
        _same_words(f"{name}: surf map as loaded", g.cubes("surf"), loaded[1])
        for k, (pose, cl, sl) in enumerate(case.steps):
            assert g.insert(cl, sl, pose) == loamx.OK
            st = _check_map(f"{name} step {k}", g, steps[k])
            assert st["iterations"] == 0
    finally:
        g.close()


# ---- the process path --------------------------------------------------------------------------------------------------------------
_TRAJ = {}


def _trajectory_model(orc):
    """the model's map, sizes and surround cloud after every step of the trajectory — computed once, shared, never written to"""
    if not _TRAJ:
        seed, steps = rc.trajectory()
        m = rm.RollingMap(orc)
        m.load_cubes(*seed)
        out = []
        for kind, pose, c, s in steps:
            m.update(pose, c, s)
            out.append(dict(corner=m.pts[0].copy(), surf=m.pts[1].copy(), stats=dict(m.stats), surround=m.surround()))
        _TRAJ["seed"], _TRAJ["steps"], _TRAJ["model"] = seed, steps, out
    return _TRAJ["seed"], _TRAJ["steps"], _TRAJ["model"]


def _step(g, where, step, want, processed):
    """one step of the trajectory on one handle; returns the words it leaves (maps, and the surround cloud when one was due)"""
    kind, pose, c, s = step
    if kind == "insert":
        assert g.insert(c, s, pose) == loamx.OK
        _check_map(where, g, want)
        return [g.cubes("corner"), g.cubes("surf")]
    g.update_odometry(pose)
    rcode, _ = g.process(c, s)
    assert rcode == loamx.OK
    st = g.stats()
    tobe = g.transform("tobe")
    assert st["sel"] == 0, f"{where}: {st['sel']} rows were selected"                       # preconditions: the pose stays the guess,
    assert np.array_equal(tobe, pose) and np.array_equal(tobe[3:].view(np.uint32), pose[3:].view(np.uint32)), f"{where}: {tobe}"   # which is the odometry pose
    _check_map(where, g, want)
    left = [g.cubes("corner"), g.cubes("surf")]
    due = processed % 5 == 1                       # the first processed frame and every fifth after it; insert() calls do not count
    assert g.has_fresh_map() == due, where
    if due:
        sur = g.surround()
        _same_words(f"{where}: surround cloud", sur, want["surround"])
        left.append(sur)
    return left


def _run_trajectory(orc, g, snapshot_after=None, tmp_path=None):
    seed, steps, model = _trajectory_model(orc)
    g.load_cubes(*seed)
    handles, left, processed = [g], [], 0
    for k, step in enumerate(steps):
        processed += step[0] == "process"
        words = [_step(h, f"handle {i} step {k} ({step[0]})", step, model[k], processed) for i, h in enumerate(handles)]
        for w in words[1:]:
            assert len(w) == len(words[0]) and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(w, words[0]))
        left.append(words[0])
        if k == snapshot_after:
            path = str(tmp_path / "map.loamx")
            g.save_snapshot(path)
            r = loamx.LaserMapping()
            r.load_snapshot(path)
            handles.append(r)
    for h in handles[1:]:
        h.close()
    return left


def test_process_path_with_speculation_hits_a_miss_and_a_shift(orc):
    g = loamx.LaserMapping()
    with_spec = _run_trajectory(orc, g)
    hits, misses = g.speculation()
    g.close()
    assert hits >= 2 and misses >= 1, (hits, misses)
    assert "LOAMX_MAP_NO_SPECULATION" not in os.environ
    os.environ["LOAMX_MAP_NO_SPECULATION"] = "1"
    try:
        g = loamx.LaserMapping()
    finally:
        del os.environ["LOAMX_MAP_NO_SPECULATION"]
    without = _run_trajectory(orc, g)
    assert g.speculation() == (0, 0)
    g.close()
    assert len(with_spec) == len(without)
    for a, b in zip(with_spec, without):
        assert len(a) == len(b) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def test_snapshot_in_the_middle_continues_word_for_word(orc, tmp_path):
    """saved after the fifth step (four processed frames, one insert), loaded into a fresh handle: both continue through the miss, the
    shift and the surround frames and leave the model's words"""
    g = loamx.LaserMapping()
    _run_trajectory(orc, g, snapshot_after=4, tmp_path=tmp_path)
    g.close()
