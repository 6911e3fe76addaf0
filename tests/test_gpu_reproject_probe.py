"""GPU: the sweep re-projection kernels on their own (loamx_reproject_probe) against tests/reproject_model.py at the cases of
tests/reproject_cases.py — points, ring-first table, order stamp and folded bounds.

The tolerance of the general class is measured, not chosen.  KAPPA = 3.5: the oracle's worst deviation from the float64 model over the
general-class cases is 3.475 x 2^-24 x (|x| + |y| + |z| + |T.pos|_1 + |shift|_1) (tests/test_reproject_cases_cpu.py measures it
again on every run).  The kernels get DEVICE_FACTOR = 4 times that, 14 x 2^-24 x scale: the device's sincosf at <= 2 ulp against the
host's <= 1, and three dependent per-point rotations.  Worst ratio observed on an MI355X: 3.475 for transformToEnd (general_K1_n4097;
the other three cases 3.26 - 3.40) and 2.956 for transformToStart (general_K6_ns3), in the same unit as KAPPA — the device sits where
the oracle sits, a quarter of its bound.

Seeded mistakes in scratch builds of odometry.hip, one MI355X run of this module each (every one must fail named cases):
  (i)   lane 0 of a wave treated as first in its cloud (the predecessor not re-read)
  (ii)  params[lo % ns] -> params[0]
  (iii) - P.shift -> + P.shift
  (iv)  the IMU start rotation applied Y-X-Z instead of Z-X-Y
  (v)   prev > ring -> prev > ring + 1
The cases each of them failed are listed in CHANGELOG.md."""
import numpy as np
import pytest

import reproject_cases as rc
import reproject_model as rm
from loam_velodyne_amd import loamx
from test_reproject_cases_cpu import call_refused, refusals

pytestmark = pytest.mark.gpu

WORST_DEVICE_RATIO = 3.475     # observed on an MI355X (see above); written down, not asserted: the assertion is DEVICE_FACTOR * KAPPA
CASES = rc.all_cases()
ids = lambda c: c.name
VARIANTS = {"fused": loamx.REPROJECT_FUSED, "single": loamx.REPROJECT_SINGLE, "copy": loamx.REPROJECT_COPY, "gather": loamx.REPROJECT_GATHER}
_RUNS = {}


def of(*cls):
    return [c for c in CASES if c.cls in cls]


def run(case, flags=0):
    """one probe call per (case, flags), shared by the tests and left unchanged"""
    key = (case.name, flags)
    if key not in _RUNS:
        _RUNS[key] = loamx.reproject_probe(case.pts, case.off, case.params, epoch=case.epoch, n_corner_all=case.n_corner_all, flags=flags,
                                           ring_first=case.table_in, bounds=case.bounds_in)
    return _RUNS[key]


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_table(case, got, w_out, table_in):
    table, choices = rm.ring_table(w_out, case.off, case.epoch, table_in)
    bad = [(c, r, hex(int(got[c, r])), hex(int(table[c, r]))) for c, r in zip(*np.nonzero(got != table)) if (c, r) not in choices]
    assert not bad, f"{case.name}: (cloud, ring, got, model) {bad[:8]}"
    for (c, r), admissible in choices.items():
        assert int(got[c, r]) in admissible, (case.name, c, r, hex(int(got[c, r])))


def check_bounds(case, got, out, bounds_in):
    want = rm.bounds(out, case.off, bounds_in)
    g, w = rm.dec_f32(got), rm.dec_f32(want)      # by value: a tie between -0 and +0 may come out with either sign
    same = (g == w) | ((got == want))
    assert same.all(), f"{case.name}: clouds {sorted(set(np.nonzero(~same)[0].tolist()))[:8]}"


# ---- exact class (and everything else with a zero rotation): word for word ---------------------------------------------------
@pytest.mark.parametrize("case", of("exact", "order", "bounds"), ids=ids)
def test_batch_kernel_equals_the_f32_model_word_for_word(case):
    r = run(case)
    want = rm.batch(rm.to_end_f32, case.pts, case.off, case.params)
    diff = np.nonzero((words(r["out"]) != words(want)).any(axis=1))[0]
    assert diff.size == 0, f"{case.name}: {diff.size} points differ, first {diff[:5]}: {r['out'][diff[:2]]} vs {want[diff[:2]]}"
    # the table, the stamp and the bounds ride on the same launch: exact in every case
    check_table(case, r["ring_first"], want[:, 3], case.table_in)
    check_bounds(case, r["bounds"], want, case.bounds_in)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_every_variant_equals_the_batch_kernel_word_for_word(case, variant):
    a, b = run(case), run(case, VARIANTS[variant])
    assert np.array_equal(words(a["out"]), words(b["out"]))
    if variant == "fused":      # the same launch with two sources: the table and the bounds hold against the model as well
        check_table(case, b["ring_first"], a["out"][:, 3], case.table_in)
        check_bounds(case, b["bounds"], a["out"], case.bounds_in)
    else:                       # no table, no bounds: the caller's words come back
        assert np.array_equal(b["ring_first"], case.table_in) and np.array_equal(b["bounds"], case.bounds_in)


@pytest.mark.parametrize("case", of("exact", "order", "bounds"), ids=ids)
def test_to_start_equals_the_f32_model_word_for_word(case):
    r = run(case, loamx.REPROJECT_TO_START)
    want = rm.batch(rm.to_start_f32, case.pts, case.off, case.params, passthrough=False)
    assert np.array_equal(words(r["out"]), words(want))


# ---- order class and bounds: what the fast path's premises are -----------------------------------------------------------------
def test_epoch_sequence_on_one_table():
    table = np.full((2, rm.RF_N), rc.FILL, np.uint32)
    model = table.copy()
    for case in rc.epoch_sequence():
        r = loamx.reproject_probe(case.pts, case.off, case.params, epoch=case.epoch, ring_first=table, bounds=case.bounds_in)
        w_out = rm.batch(rm.to_end_f32, case.pts, case.off, case.params)[:, 3]
        check_table(case, r["ring_first"], w_out, table)
        table = r["ring_first"]
        model, _ = rm.ring_table(w_out, case.off, case.epoch, model)
    assert table[0, rm.RF_N - 1] == 254 and table[1, rm.RF_N - 1] == rc.FILL
    assert table[0, 10] >> 24 == 254 and table[0, 15] >> 24 == 255 and table[0, 20] >> 24 == 1


@pytest.mark.parametrize("name", ["bounds_straddling", "order_descent_at_64", "exact_K6_ns3"])
def test_table_and_bounds_can_each_be_left_out(name):
    case = next(c for c in CASES if c.name == name)
    full = run(case)
    no_rf = run(case, loamx.REPROJECT_NO_RING_TABLE)
    no_bb = run(case, loamx.REPROJECT_NO_BOUNDS)
    neither = run(case, loamx.REPROJECT_NO_RING_TABLE | loamx.REPROJECT_NO_BOUNDS | loamx.REPROJECT_FUSED)
    for r in (no_rf, no_bb, neither):
        assert np.array_equal(words(r["out"]), words(full["out"]))
    assert np.array_equal(no_rf["ring_first"], case.table_in) and np.array_equal(no_bb["bounds"], case.bounds_in)
    assert np.array_equal(neither["ring_first"], case.table_in) and np.array_equal(neither["bounds"], case.bounds_in)
    assert np.array_equal(no_bb["ring_first"], full["ring_first"])
    check_bounds(case, no_rf["bounds"], full["out"], case.bounds_in)


# ---- general class: the measured bound -----------------------------------------------------------------------------------------
def device_ratio(case, got, f64):
    worst = 0.0
    for c in range(case.K):
        a, b = int(case.off[c]), int(case.off[c + 1])
        if b > a:
            P = case.params[c % case.ns]
            err = np.abs(got[a:b, :3].astype(np.float64) - f64(case.pts[a:b], P)[:, :3]).max(axis=1)
            worst = max(worst, float((err / (2.0 ** -24 * rm.scale(case.pts[a:b], P))).max()))
    return worst


@pytest.mark.parametrize("case", of("general"), ids=ids)
def test_general_class_stays_within_the_measured_bound(case):
    end, start = run(case), run(case, loamx.REPROJECT_TO_START)
    r_end, r_start = device_ratio(case, end["out"], rm.to_end_f64), device_ratio(case, start["out"], rm.to_start_f64)
    print(f"{case.name}: device ratio to_end {r_end:.3f}, to_start {r_start:.3f} (KAPPA {rm.KAPPA}, bound {rm.DEVICE_FACTOR * rm.KAPPA})")
    assert max(r_end, r_start) <= rm.DEVICE_FACTOR * rm.KAPPA
    assert np.array_equal(words(end["out"][:, 3]), words(np.trunc(case.pts[:, 3]))), ".w is exactly the truncated ring"
    assert np.array_equal(words(start["out"][:, 3]), words(case.pts[:, 3]))
    check_table(case, end["ring_first"], end["out"][:, 3], case.table_in)
    check_bounds(case, end["bounds"], end["out"], case.bounds_in)


# ---- the public path: the same kernels behind LaserOdometry --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["general_K1_n4097", "general_K4_ns1_n257"])
def test_public_path_stays_within_the_same_bound(name):
    case = next(c for c in CASES if c.name == name)
    P, ang = case.params[0], case.imu_angles[0]
    t12 = np.concatenate([ang, P["shift"], np.zeros(3, np.float32)]).astype(np.float32)
    want = rm.to_end_f64(case.pts, P)
    lim = rm.bound(case.pts, P, rm.DEVICE_FACTOR)[:, None]
    # (the handle makes its sine / cosine words with the host's sinf / cosf: within an ulp of the record's, which the bound's
    # KAPPA — the oracle does the same — has measured in)
    od = loamx.LaserOdometry(scan_period=float(P["scan_period"]))
    od.set_transform(P["T"])
    od.update_imu(t12)
    got = od.transform_to_end(case.pts)
    assert (np.abs(got[:, :3] - want[:, :3]) <= lim).all() and np.array_equal(got[:, 3], np.trunc(case.pts[:, 3]))
    # the batch kernel inside the real pass: too few points to optimise (test_too_few_points_guard), so the second sweep's clouds
    # are re-projected with the transform as set (zero IMU velocity leaves it alone)
    nc = min(9, case.n // 2)
    f = dict(sharp=case.pts[:4], less_sharp=case.pts[:nc], flat=case.pts[nc:nc + 4], less_flat=case.pts[nc:nc + 90])
    od.process(f)
    od.set_transform(P["T"])
    od.process(f)
    assert od.stats()["iterations"] == 0 and np.array_equal(od.transform, P["T"])
    corner, surf = od.last_clouds()
    for got, src in ((corner, f["less_sharp"]), (surf, f["less_flat"])):
        assert len(got) == len(src)
        assert (np.abs(got[:, :3] - rm.to_end_f64(src, P)[:, :3]) <= rm.bound(src, P, rm.DEVICE_FACTOR)[:, None]).all()
        assert np.array_equal(got[:, 3], np.trunc(src[:, 3]))
    od.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", refusals(), ids=[r[0] for r in refusals()])
def test_refusals_with_a_device(name, kw):
    assert call_refused(loamx, kw) == loamx.E_INVALID


def test_no_points_needs_no_launch():
    case = next(c for c in CASES if c.name == "exact_n0")
    for flags in (0, 1, 2, 3, 4, 5):
        r = loamx.reproject_probe(case.pts, case.off, case.params, flags=flags, ring_first=case.table_in, bounds=case.bounds_in)
        assert len(r["out"]) == 0 and np.array_equal(r["ring_first"], case.table_in) and np.array_equal(r["bounds"], case.bounds_in)
