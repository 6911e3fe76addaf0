"""CPU: every case of tests/featring_cases.py is the edge it claims to be (analyse() recomputes the facts from the model's data the way
k_feat_ring derives them), the model of the sequential walk equals the oracle and the reference's own compiled BasicScanRegistration
word for word on every case, the kernel's settlement rule restated over the model's data gives the sequential walk's picks, and the
cases have teeth: every one-line mutant of the model differs from the oracle on the cases named for it."""
import numpy as np
import pytest

import featring_cases as fc
import oracle_py as op

CASES = fc.cases()
ANALYSIS = {}

# mutant -> the cases written to catch it.  Asserted both ways: each listed case differs under the mutant, and every mutant that is
# not provably equivalent has a case.
MUTANT_CASES = {
    "ties_reversed": ("ties, all zero, region of 64", "ties, equal positive curvature, cr 5", "sort 505, all equal", "sort 56, all zero"),
    "ties_corner_first": ("ties, two spikes, max_sharp 1", "ties, five spikes across max_less_sharp", "ties, five spikes, cr 16", "sort 249, organ pipe"),
    "float_compares": ("double compare, gap, step^2 == float(0.05)", "double compare, occlusion, step^2 == float(0.1)",
                       "double compare, beam test, step^2 == float(float(0.0002) * dis)"),
    "thr_inclusive": ("threshold at the tied curvature",),
    "no_skip_round": ("rounds, corner walk, 64 inadmissible first", "rounds, corner walk, 128 inadmissible first", "rounds, flat walk, 64 inadmissible first",
                      "rounds, flat walk, 127 inadmissible first"),
    "regions_independent": ("settlement, one region remade", "settlement, cascade", "settlement, mark withdrawn",
                            "settlement, cascade across the group boundary, 13 regions"),
    "no_cascade": ("settlement, cascade", "settlement, mark added", "settlement, mark withdrawn", "settlement, cascade across the group boundary, 7 regions"),
    "marks_ignore_gaps": ("gap break beside the pick", "gap break on a region boundary", "double compare, gap, step^2 == float(0.05)"),
    "mask_off_by_one": ("mask, far to near one beyond the last index",),
    "s0_zero": (),   # equivalent: the regions of a ring do not depend on where it starts (fc.EQUIVALENT_MUTANTS, test_regions_do_not_depend_on_the_start)
}


def _analysis(case):
    if case.name not in ANALYSIS:
        ANALYSIS[case.name] = fc.analyse(case)
    return ANALYSIS[case.name]


_by_name = lambda cases: pytest.mark.parametrize("case", cases, ids=lambda c: c.name)


def _same(a, b):
    return fc.first_difference(a, b) is None


def _differs(orc, case, mutant):
    return not _same(fc.model(case, mutant)["clouds"], fc.cached_oracle(orc, case))


def test_names_are_unique_and_rows_name_their_source():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    for c in CASES:
        for r, ring in enumerate(c.rings):
            assert len(ring) < 8192
            assert all(fc.source_of(row) == (r, k) for k, row in list(enumerate(ring))[:: max(1, len(ring) // 7)])
            assert len(np.unique(ring[:, 3])) == len(ring)


def _check_region_claims(case, reg, cl):
    for key in ("corner", "flat"):
        if key in cl:
            assert reg[key] == cl[key], (key, reg[key])
    for key in ("corner_lead", "corner_empty_rounds", "flat_lead", "flat_empty_rounds", "corner_stop_lane"):
        if key in cl:
            assert reg[key] == cl[key], (key, reg[key])
    if "corner_first_lane" in cl:
        assert reg["corner_lanes"][0] == cl["corner_first_lane"]
    if "flat_first_lane" in cl:
        assert reg["flat_lanes"][0] == cl["flat_first_lane"]
    if "region_size" in cl:
        assert reg["size"] == cl["region_size"]
    if "all_equal" in cl:
        assert len(reg["ties"]) == 1 and len(reg["ties"][0]["members"]) == reg["size"]
        if cl["all_equal"] is not True:
            assert reg["ties"][0]["value"] == cl["all_equal"]
        if cl.get("positive"):
            assert 0 < reg["ties"][0]["value"] < case.thr
    if cl.get("straddles"):
        assert any(cl["straddles"] in t["straddles"] for t in reg["ties"]), [t["straddles"] for t in reg["ties"]]
    if "tie_of" in cl:
        assert any(len(t["members"]) == cl["tie_of"] and t["value"] > case.thr for t in reg["ties"])
    if cl.get("picks_nothing"):
        assert reg["corner"] == [] and reg["flat"] == [] and reg["corner_end"] == "exhaustion" and reg["corner_empty_rounds"] >= 4
        assert reg["flags_end"].all()
    if cl.get("stop_in_round"):
        assert reg["corner"] and reg["corner_end"] == "break" and reg["corner_stop_lane"] > 0 and reg["corner_free_behind_stop"] > 0
    if "stretch" in cl:
        tie = [t for t in reg["ties"] if t["value"] == cl["value"]][0]
        assert tie["at_threshold"] == (cl["stretch"] == "neither") and len(tie["members"]) >= 30
        picked = {"corner": set(reg["corner"]), "flat": set(reg["flat"])}
        members = set(int(m) for m in tie["members"])
        assert bool(members & picked["corner"]) == (cl["stretch"] == "corner") and bool(members & picked["flat"]) == (cl["stretch"] == "flat")
        if cl["stretch"] == "neither":
            assert reg["corner_end"] == "break" and reg["flat_end"] == "break"


@_by_name(CASES)
def test_case_is_what_it_claims(case):
    a, cl = _analysis(case), case.claims
    assert len(a) == len(case.rings) and all(r["accepted"] for r in a)
    live = [r for r in a if r["processed"]]
    for r in live:
        if r["simple"]:
            assert r["settle_equals_walk"], "the settlement rule does not give the sequential walk's picks"
    if "ring_lens" in cl:
        assert case.sizes() == cl["ring_lens"]
    if "simple" in cl:
        assert [r["simple"] for r in a] == cl["simple"]
    if "sortP" in cl:
        assert a[0]["sortP"] == cl["sortP"]
    first = live[0] if live else None
    if "designed" in cl:
        first = a[cl["designed"]]
        assert first["s0"] == cl["start"] and first["processed"] and first["simple"]
    if first is not None and first["regions"] and case.nreg == 1:
        _check_region_claims(case, first["regions"][0], cl)
    # settlement
    simple = [r for r in live if r["simple"]]
    if any(k in cl for k in ("remade", "crossed", "added", "withdrawn", "unpicked_only")):
        for r in simple:
            s = fc.settlement_summary(r)
            for key in ("remade", "crossed", "added", "withdrawn", "unpicked_only"):
                if key in cl:
                    assert s[key] == cl[key], (key, s[key])
    if cl.get("some_remade"):
        s = fc.settlement_summary(simple[0])
        assert len(s["remade"]) >= 2 and s["out_changed"]
        sizes = [n for _, _, n in simple[0]["bounds"]]
        assert min(sizes) >= case.cr
    # masks
    if "branch" in cl:
        got = first["branch"]
        assert set(got) == set(cl["branch"]), got
        for k, b in cl["branch"].items():
            assert b in got[k], (k, got[k])
    if "flagged" in cl:
        assert sorted(np.flatnonzero(first["flags0"])) == sorted(cl["flagged"]), np.flatnonzero(first["flags0"])
    if "unflagged" in cl:
        assert not first["flags0"][cl["unflagged"]].any()
    if "min_chunks" in cl:
        assert first["staged"] and first["chunks"] >= cl["min_chunks"] and first["chunk"] == cl["chunk"]
        for k, b in cl["branch"].items():   # the flagged window lies across a chunk boundary
            lo, hi = (k - case.cr, k) if b == "occl_back" else (k + 1, k + 1 + case.cr)
            assert lo // first["chunk"] != hi // first["chunk"] or k // first["chunk"] != (k + 1) // first["chunk"], (k, first["chunk"])
    # the double comparisons
    if "step" in cl:
        k, const = cl["step"]
        v = fc.point_pass(case.rings[0], case.cr)["step"][k]
        on = cl.get("is_gap", cl.get("enters"))
        assert v == (np.float32(const) if on else np.nextafter(np.float32(const), np.float32(0)))
        assert (float(v) > const) == on and not v > np.float32(const)   # on the value the double and the float32 comparison disagree
    if "is_gap" in cl:
        assert bool(first["gaps"][cl["step"][0]]) == cl["is_gap"]
        if cl["flat_has"] is not None:
            assert cl["flat_has"] in first["regions"][0]["flat"]
        if cl["flat_lacks"] is not None:
            assert cl["flat_lacks"] not in first["regions"][0]["flat"]
    if "enters" in cl:
        assert (cl["step"][0] in first["branch"]) == cl["enters"]
    if "beam_at" in cl:
        assert "beam" in first["branch"][cl["beam_at"]] and first["beam_flagged"] != []
    # gap breaks
    if "cuts" in cl:
        assert first["regions"][0]["cuts"][:len(cl["cuts"])] == cl["cuts"], first["regions"][0]["cuts"]
        assert first["regions"][0]["corner"][:2] == cl["corner_starts"]
    if "boundary_gap" in cl:
        g = cl["boundary_gap"]
        assert first["gaps"][g - 1] and any(s == g for _, s, _ in first["bounds"])
        before, after = fc.region_of(case, 0, g - 1, a), fc.region_of(case, 0, g, a)
        assert g - 1 - before["start"] in before["corner"] and g - after["start"] in after["corner"]   # both sides of the gap are picked
        assert any(e == g - 1 - before["start"] and nf == 0 for e, nf, nb in before["cuts"])
    if cl.get("first_last"):
        regs = first["regions"]
        assert 0 in regs[0]["corner"] and regs[-1]["size"] - 1 in regs[-1]["corner"]
        assert regs[0]["start"] == case.cr and regs[-1]["start"] + regs[-1]["size"] - 1 == first["len"] - case.cr - 2


def test_the_set_reaches_every_path():
    regs = [reg for c in CASES for r in _analysis(c) if r["processed"] for reg in r["regions"]]
    rings = [r for c in CASES for r in _analysis(c)]
    assert {64, 128, 256, 512, 1024} <= {r["sortP"] for r in rings}
    assert any(r["processed"] and not r["simple"] for r in rings) and any(not r["processed"] for r in rings) and any(r["len"] == 0 for r in rings)
    assert {0, 1, 2} <= {reg["corner_empty_rounds"] for reg in regs} and {0, 1, 2} <= {reg["flat_empty_rounds"] for reg in regs}
    assert {0, 1, 63} <= {reg["corner_lanes"][0] for reg in regs if reg["corner"]} and {0, 1, 63} <= {reg["flat_lanes"][0] for reg in regs if reg["flat"]}
    assert {"break", "limit", "exhaustion"} <= {reg["corner_end"] for reg in regs}
    assert {"break", "limit"} <= {reg["flat_end"] for reg in regs}
    assert {"max_sharp", "max_less_sharp", "max_flat"} <= {s for reg in regs for t in reg["ties"] for s in t["straddles"]}
    assert any(t["at_threshold"] for reg in regs for t in reg["ties"])
    branches = {b for r in rings if r["processed"] for bs in r["branch"].values() for b in bs}
    assert {"equal_depth", "far_to_near", "near_to_far", "occl_back", "occl_fwd", "wide", "beam", "beam_skipped"} <= branches
    summaries = [fc.settlement_summary(r) for r in rings if r["simple"]]
    for key in ("remade", "crossed", "added", "withdrawn", "unpicked_only"):
        assert any(s[key] for s in summaries), key
    assert any(12 in s["crossed"] for s in summaries) and any(s["remade"] == [1, 2, 3, 4, 5] for s in summaries)
    assert {1, 5, fc.MAX_CR} <= {c.cr for c in CASES} and {1, 6, 7, 12, 13, 64} <= {c.nreg for c in CASES}


def test_regions_do_not_depend_on_the_start():
    """(s0 + cr)(nreg - j) + (e0 - cr) j = nreg * s0 + ...: the ring's start leaves the quotient's floor alone.  So the start-index
    family has ONE partition, `s0_zero` is an equivalent mutant, and what the family pins is the device's handling of the offset."""
    for nreg in (1, 6, 7, 13, 64):
        for cr in (1, 5, 16):
            for n in (2 * cr + 2, 40, 300, 301, 1000):
                want = fc.region_bounds(0, n, cr, nreg)
                for s0 in (1, 2, 5, 12, 13, 4097, 2**31 + 5):
                    assert fc.region_bounds(s0, n, cr, nreg) == want
    fam = [c for c in CASES if c.name.startswith("start index")]
    assert [c.claims["start"] for c in fam] == list(fc.START_OFFSETS)
    parts = {tuple(_analysis(c)[1]["bounds"]) for c in fam}
    picks = {tuple(tuple(reg["corner"]) + tuple(reg["flat"]) for reg in _analysis(c)[1]["regions"]) for c in fam}
    assert len(parts) == 1 and len(picks) == 1
    assert sum(len(reg["corner"]) for reg in _analysis(fam[0])[1]["regions"]) >= 8   # (the designed ring has picks to compare)


@_by_name(CASES)
def test_model_equals_the_oracle(orc, case):
    d = fc.first_difference(fc.cached_model(case)["clouds"], fc.cached_oracle(orc, case))
    assert d is None, d


@pytest.mark.skipif(not op.RefScanRegistration.available(), reason="oracle/_ref not built")
@_by_name(CASES)
def test_compiled_reference_equals_the_oracle(orc, case):
    ref = op.RefScanRegistration(**case.oracle_config()).process(case.cloud(), case.sizes())
    d = fc.first_difference(ref, fc.cached_oracle(orc, case))
    assert d is None, d


@pytest.mark.parametrize("mutant", fc.MUTANTS)
def test_mutant_is_caught_by_its_cases(orc, mutant):
    names = MUTANT_CASES[mutant]
    if mutant in fc.EQUIVALENT_MUTANTS:
        assert names == ()
        for c in CASES:
            if c.name.startswith("start index") or c.name == "mixed batch":
                assert not _differs(orc, c, mutant), c.name
        return
    assert names, f"no case pins {mutant}"
    for n in names:
        assert _differs(orc, fc.by_name(n, CASES), mutant), (mutant, n)


def test_mutant_table_is_complete():
    assert set(MUTANT_CASES) == set(fc.MUTANTS)
    for c in CASES:
        for mu in c.claims.get("caught_by", ()):
            assert mu in fc.MUTANTS


def test_settlement_mutants_differ_exactly_where_claimed(orc):
    fam = [c for c in CASES if c.name.startswith("settlement") and "caught_by" in c.claims]
    assert len(fam) >= 9
    for c in fam:
        got = {mu for mu in ("regions_independent", "no_cascade") if _differs(orc, c, mu)}
        assert got == set(c.claims["caught_by"]) & {"regions_independent", "no_cascade"}, (c.name, got)
    by = {c.name: c for c in fam}
    assert by["settlement, marks on unpicked points only"].claims["caught_by"] == ()
    assert "no_cascade" not in by["settlement, one region remade"].claims["caught_by"]


@_by_name([c for c in CASES if "caught_by" in c.claims and not c.name.startswith("settlement")])
def test_cases_catch_what_they_say(orc, case):
    """the pairs around a constant: the case ON the value is caught by the mutant, its neighbour one ulp away by none of them"""
    for mu in ("float_compares", "marks_ignore_gaps", "thr_inclusive", "mask_off_by_one"):
        if mu in case.claims["caught_by"] or case.claims["caught_by"] == ():
            assert _differs(orc, case, mu) == (mu in case.claims["caught_by"]), mu


def test_reuse_sequence():
    seq = [fc.by_name(n, CASES) for n in fc.REUSE_ORDER]
    assert seq[0] is seq[-1] and len({(c.cr, c.nreg) for c in seq}) >= 4
    assert len({(c.max_sharp, c.max_less_sharp, c.max_flat) for c in seq}) >= 3 and {64, 1024} <= {_analysis(c)[0]["sortP"] for c in seq}
