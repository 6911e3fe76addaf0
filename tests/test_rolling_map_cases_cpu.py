"""CPU: every generated case of the rolling map's update (tests/rolling_map_cases.py) reaches the path it claims, by the model's facts
(tests/rolling_map_model.py), and the model equals the oracle's LaserMapping — run with no iteration and the pose as its odometry, so
that transformTobeMapped is the pose bit for bit — cube by cube, sequence for sequence, as uint32 words; where the reference's own
mapping unit is built, the cases that start from an empty handle equal it too.

Conditions on the inputs, asserted here (they are not tolerances): every field-of-view test of every case stays 1e-2 away from its
threshold, no coordinate of any input or result is -0.0, and the cases whose surround cloud is compared lie on a 2^-6 m lattice with
at most 16 points per voxel, so that the order of summation cannot matter."""
import numpy as np
import pytest

import oracle_py as op
import rolling_map_cases as rc
import rolling_map_model as rm


def _words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _no_negative_zero(a):
    a = np.asarray(a)
    return not (np.signbit(a) & (a == 0)).any()


def test_every_family_is_there():
    for n in (1, 7, 8, 9, 2047, 2048, 2049, 4097, 65 * 2048 + 1):
        assert f"split_{n}" in rc.BUILDERS
    for n in (0, 1, 255, 256, 257, 64 * 256 + 1):
        assert f"insert_{n}" in rc.BUILDERS
    for k in ("split_all_valid", "split_all_rest", "split_all_dropped", "split_per_tile", "split_corner_empty", "split_surf_empty", "split_both_empty",
              "insert_all_valid", "insert_all_rest", "insert_all_dropped", "insert_runs", "insert_corner_none", "insert_input_larger",
              "append_lead_mid_trail", "append_all_empty", "append_one_slot", "append_first_last", "hist_grid_stride", "faces_x", "faces_y", "faces_z",
              "shift_xp", "shift_xm", "shift_yp", "shift_ym", "shift_zp", "shift_zm", "shift_several", "shift_threshold_on", "shift_threshold_below",
              "shift_out_and_back", "shift_from_empty", "sequence_growing", "sequence_lattice"):
        assert k in rc.BUILDERS
    assert len(rc.NAMES) == 49


@pytest.mark.parametrize("name", rc.NAMES)
def test_case_is_what_it_claims(orc, name):
    case = rc.get(name)
    loaded, steps = rc.model(orc, name)
    facts = [s["facts"] for s in steps]
    assert bool(case.check(facts)), case.claim
    for f in facts:
        assert min(f["min_check1"], f["min_check2"]) > 1e-2, "a field-of-view test too close to its threshold"
    for a in list(case.seed) + [x for st in case.steps for x in st] + [s[k] for s in steps for k in ("corner", "surf")]:
        assert _no_negative_zero(a)
    if case.lattice:
        for s in steps:
            for k in ("corner", "surf"):
                assert np.array_equal(s[k][:, :3] * 64, np.round(s[k][:, :3] * 64))
            allp = np.concatenate([s["corner"], s["surf"]])
            _, cnt = np.unique(np.floor(allp[:, :3] * (np.float32(1) / np.float32(0.2))), axis=0, return_counts=True)
            assert cnt.max() <= 16


def test_shift_threshold_is_the_boundary():
    on, below = rc.get("shift_threshold_on").steps[0][0], rc.get("shift_threshold_below").steps[0][0]
    assert on[3] == np.float32(375) and below[3] == np.nextafter(np.float32(375), np.float32(0))


def test_cube_abs_at_the_faces():
    v = np.array([-25, 25, 75, -75, np.nextafter(np.float32(-25), np.float32(-100)), np.nextafter(np.float32(25), np.float32(0)), -525, 524.99], np.float32)
    assert rm.cube_abs(v).tolist() == [0, 1, 2, -2, -1, 0, -11, 10]


def _run_reference_side(h, case, with_stats):
    """the oracle (or the reference's own unit) through the case: the pose as odometry, bef / aft zero, no iteration"""
    out = []
    for pose, cl, sl in case.steps:
        h.set_transform("bef", np.zeros(6, np.float32))
        h.set_transform("aft", np.zeros(6, np.float32))
        h.set_inputs(cl, sl, np.zeros((0, 4), np.float32), pose)
        assert h.process()
        tobe = h.transform("tobe")
        assert np.array_equal(tobe, pose) and np.array_equal(_words(tobe[3:]), _words(pose[3:]))
        out.append(dict(corner=h.cloud("corner_cubes"), surf=h.cloud("surf_cubes"), stats=h.stats() if with_stats else None,
                        surround=h.cloud("surround_ds") if h.has_fresh_map() else None))
    return out


def _compare(case, steps, ref, what):
    n_surround = 0
    for k, (m, r) in enumerate(zip(steps, ref)):
        for t, which in enumerate(("corner", "surf")):
            assert m["grouped"][t].shape == r[which].shape, (what, k, which)
            assert np.array_equal(_words(m["grouped"][t]), _words(r[which])), (what, k, which)
            assert _no_negative_zero(r[which])
        if r["stats"] is not None:
            assert {key: r["stats"][key] for key in m["stats"]} == m["stats"], (what, k)
        if case.lattice and r["surround"] is not None:
            n_surround += 1
            assert m["surround"].shape == r["surround"].shape and np.array_equal(_words(m["surround"]), _words(r["surround"])), (what, k, "surround")
    return n_surround


@pytest.mark.parametrize("name", rc.NAMES)
def test_the_model_equals_the_oracle(orc, name):
    case = rc.get(name)
    loaded, steps = rc.model(orc, name)
    o = op.LaserMapping(orc, maxIterations=0)
    o.load_cubes(*case.seed)
    n_surround = _compare(case, steps, _run_reference_side(o, case, True), "oracle")
    if case.lattice:
        assert n_surround == (2 if len(case.steps) > 5 else 1)


@pytest.mark.parametrize("name", [n for n in rc.NAMES if rc.get(n).from_empty])
def test_the_model_equals_the_reference_mapping_unit(orc, name):
    if not op.RefLaserMapping.available():
        pytest.skip("the reference's own mapping unit is not built here")
    case = rc.get(name)
    loaded, steps = rc.model(orc, name)
    _compare(case, steps, _run_reference_side(op.RefLaserMapping(maxIterations=0), case, False), "reference")


def test_the_trajectory_selects_no_row(orc):
    """the process path's precondition: every feature is 1.5 m or more from every point the map holds when it arrives"""
    seed, steps = rc.trajectory()
    m = rm.RollingMap(orc)
    m.load_cubes(*seed)
    kinds = [s[0] for s in steps]
    assert kinds.count("process") == 11 and kinds.count("insert") == 2
    shifted = 0
    for kind, pose, c, s in steps:
        have = np.concatenate([m.pts[0], m.pts[1]])
        for f in (c, s):
            q = rm.to_map_zero_angles(f, pose[3:])[:, :3].astype(np.float64)
            d2 = ((q[:, None, :] - have[None, :, :3].astype(np.float64)) ** 2).sum(axis=2)
            assert d2.min() >= 1.5 ** 2
        facts = m.update(pose, c, s)
        shifted += any(facts["shifts"])
        assert min(facts["min_check1"], facts["min_check2"]) > 1e-2
        assert _no_negative_zero(m.pts[0]) and _no_negative_zero(m.pts[1])
    assert shifted == 1
