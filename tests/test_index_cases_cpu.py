"""CPU: every generated index case (tests/index_cases.py) is what it claims to be — recomputed from the model
(tests/submap_index_model.py): the set-up path, the growth steps, what wave_runs and cloud_bounds_update meet, where the empty clouds
are — and for every case, by brute force, the property both searches rest on: each point within cell_edge * sqrt(0.9999) of a query
lies in the 27 cells around the query's cell under the model's descriptor."""
import numpy as np
import pytest

import index_cases as ic
import submap_index_model as sm

CASES = ic.all_cases()
_MODEL = {}


def model(case):
    key = case.name[:-5] if case.flags & ic.FOLD else case.name   # (folding the bounds changes how they are gathered, not the result)
    if key not in _MODEL:
        _MODEL[key] = sm.build(case.pts, case.off, case.cell, case.flags)
    return _MODEL[key]


def test_every_family_is_there():
    names = {c.name for c in CASES}
    for n in ic.SIZES:
        assert {f"single_n{n}", f"batch_n{n}", f"single_n{n}_fold", f"batch_n{n}_fold"} <= names
    for K in ic.KS:
        assert {f"K{K}_cell1.05", f"K{K}_cell2.1", f"K{K}_cell1.05_fold", f"K{K}_cell2.1_fold"} <= names
    assert {"single_n32769", "batch_cloud8193", "single_cube1e6", "batch_K4096_20m", "empty_all_K70_fold", "rings_packed"} <= names
    paths = {c.claims["path"] for c in CASES}
    assert paths == {"single", "fused", "unfused", "unfused2"}
    assert max(c.n for c in CASES) <= 40000
    for seq in ic.sequences().values():
        assert len(seq) >= 4


def test_no_case_goes_beyond_what_the_cpu_driver_pins():
    """extents stay within the 1e6 m cube (tests/test_grid_fit.py holds grid_fit to the former loop there); the cell edges are the product's"""
    for c in CASES + [x for s in ic.sequences().values() for x in s]:
        if c.n:
            assert np.isfinite(c.pts).all() and float(np.ptp(c.pts[:, :3].astype(np.float64), axis=0).max()) <= 1e6
        assert c.cell in (0.25, 0.5, 2.0, 1.05, 2.1) and c.K <= 4096
        if c.flags & ic.SINGLE:
            assert c.K == 1 and c.n >= 1 and c.cell == 1.05 and not c.flags & ic.PACK_RING


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_is_what_it_claims(case):
    m, cl = model(case), case.claims
    assert sm.setup_path(case.off, case.flags) == cl["path"]
    assert int(m["steps"].max()) == cl.get("grows", 0), "growth steps of the coarsest cloud"
    lens = np.diff(case.off.astype(np.int64))
    if "empties" in cl:
        assert list(np.flatnonzero(lens == 0)) == cl["empties"]
    w = sm.wave_facts(m["cell"], case.off)
    if "tail_lanes" in cl:
        assert w["tail_lanes"] == cl["tail_lanes"]
    if cl.get("cut_at_wave_end"):
        assert w["cut_at_wave_end"] >= 1
    if cl.get("run_across_waves"):
        assert w["run_across_waves"] >= 1
    if "longest_run" in cl:
        assert w["longest_run"] >= cl["longest_run"] if cl["longest_run"] > 1 else w["longest_run"] == 1
    if cl.get("mixed_wave"):
        assert w["mixed_waves"] >= 1
    if "boundaries_in_wave" in cl:
        assert w["boundaries_inside_a_wave"] >= cl["boundaries_in_wave"]
    if "clouds_in_wg" in cl:
        assert w["max_clouds_in_workgroup"] >= cl["clouds_in_wg"]
    if cl.get("dedup"):
        assert w["same_cloud_waves_in_workgroup"] >= 2
    if cl.get("bbox_capped"):
        assert lens.max() > (128 if case.flags & ic.SINGLE else 32) * 256
    d = m["desc"]
    if cl.get("integer_extent"):
        mn, mx = sm.bounds(case.pts[:lens[0], :3])
        q = (mx - mn) * d[0]["inv_h"]
        assert (q == np.floor(q)).all() and (q >= 1).all() and [d[0]["nx"], d[0]["ny"], d[0]["nz"]] == [int(v) + 1 for v in q]
    if cl.get("zeros"):
        u = case.pts[:lens[0], :3].view(np.uint32)
        assert ((u == 0x80000000).any(axis=0) & (u == 0).any(axis=0)).all()
        assert (d[0][["ox", "oy", "oz"]].tolist() == np.array([-0.0] * 3, np.float32)).all() and np.signbit([d[0]["ox"], d[0]["oy"], d[0]["oz"]]).all()
    if cl.get("negative"):
        assert (case.pts[:, :3] < 0).any()
    if "rings" in cl:
        assert sorted(set((m["w"] >> 24).tolist())) == cl["rings"]
    # the model's own consistency: budget, table, cells inside their cloud's range
    K = case.K
    nc = d["ncell"].astype(np.int64)
    assert (nc == d["nx"].astype(np.int64) * d["ny"] * d["nz"]).all() and (nc <= sm.budget_of(K, bool(case.flags & ic.SINGLE))).all() and (nc >= 1).all()
    assert int(m["table"][-1]) == case.n and len(m["table"]) == int(nc.sum()) + 1 <= sm.MAX_CELLS + 1


@pytest.mark.parametrize("case", [c for c in CASES if not c.flags & ic.FOLD], ids=lambda c: c.name)
def test_the_27_cells_hold_every_point_within_the_gate(case):
    bad = sm.neighbourhood_violations(case.pts, case.off, model(case)["desc"], case.cell)
    assert not bad, f"{case.name}: {len(bad)} pairs, first (cloud, query, point) {bad[0]}"


def test_encoding_orders_floats_as_the_accumulators_need_it():
    v = np.array([-np.inf, -3.0e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.0e38, np.inf], np.float32)
    e = sm.enc_f32(v)
    assert (np.diff(e.astype(np.int64)) > 0).all() and np.array_equal(sm.dec_f32(e).view(np.uint32), v.view(np.uint32))
    assert e.min() > 0 and e.max() < 0xffffffff     # the reset words (all ones for a minimum, zero for a maximum) lose against every float


def test_sequences_change_what_the_object_was_left_with():
    s = ic.sequences()
    ks = [c.K for c in s["K_64_65_4096_2"]]
    assert ks[:4] == [64, 65, 4096, 2]
    paths = [c.claims["path"] for c in s["fused_unfused_alternating"]]
    assert all(a != b for a, b in zip(paths[:5], paths[1:5])) or paths[:4] == ["fused", "unfused", "fused", "unfused2"]
    assert [c.n for c in s["all_empty_between"]][1] == 0 and [c.n for c in s["all_empty_between"]][3] == 0
    f = [bool(c.flags & ic.FOLD) for c in s["folded_unfolded_alternating"]]
    assert f == [True, False] * 4
    big, small = s["large_then_small"][0], s["large_then_small"][1]
    assert big.n > 100 * small.n
    wide, narrow = s["wide_then_narrow"][0], s["wide_then_narrow"][1]
    assert np.ptp(wide.pts[:, 0]) > 50 * np.ptp(narrow.pts[:, 0])
