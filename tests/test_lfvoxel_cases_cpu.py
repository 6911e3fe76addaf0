"""CPU: every case of tests/lfvoxel_cases.py is the edge it claims to be (recomputed by analyse() the way k_feat_lf_voxel derives
it), the set as a whole reaches every pass count, pass-through and every per_wave, the huge-threshold handle really makes the oracle's
full ScanRegistration emit `voxel grid of p[candidates]` per ring (the premise of tests/test_gpu_lfvoxel.py), and the cases have
teeth: three subtly wrong grids each differ from the oracle on a named case."""
import numpy as np
import pytest

import lfvoxel_cases as lc
import oracle_py as op

CASES = lc.all_cases()
EXTRA = list(lc.dispatch_pair()) + [lc.mixed_batch_case(longest=4097)]
ANALYSIS = {}


def _analysis(case):
    if case.name not in ANALYSIS:
        ANALYSIS[case.name] = lc.analyse(case)
    return ANALYSIS[case.name]


_by_name = lambda cases: pytest.mark.parametrize("case", cases, ids=lambda c: c.name)


def test_candidates_of_one_region_are_the_slice():
    for cr in (1, 5):
        for n in range(0, 70):
            want = np.arange(cr, n - cr - 1) if n >= 2 * cr + 3 else np.zeros(0, np.int64)
            assert np.array_equal(lc.candidates(n, cr, 1), want), (cr, n)
        assert len(lc.candidates(4096, cr, 1)) == 4096 - 2 * cr - 1
    assert len(lc.candidates(2 * 5 + 3, 5, 1)) == 2 and len(lc.candidates(2 * 5 + 2, 5, 1)) == 0   # one candidate is unreachable


def test_candidates_of_many_regions_skip_one_point_regions():
    for nreg in (6, 13):
        for n in range(0, 400):
            c = lc.candidates(n, 5, nreg)
            assert np.all(np.diff(c) > 0) and (len(c) == 0 or (c[0] >= 5 and c[-1] <= n - 5 - 2))
            assert len(c) != 1
        # short rings lose the points of their one-point regions; long ones keep the whole span
        assert len(lc.candidates(300, 5, nreg)) == 300 - 11
        assert len(lc.candidates(nreg * 5 + 11, 5, nreg)) == nreg * 5
        assert 0 < len(lc.candidates(11 + nreg + nreg // 2, 5, nreg)) < nreg + nreg // 2   # regions of one and of two points
        assert len(lc.candidates(13, 5, nreg)) == 0 and len(lc.candidates(12, 5, nreg)) == 0   # (one region would give 2 and 0)


@_by_name(CASES + EXTRA)
def test_case_is_what_it_claims(case):
    a, cl = _analysis(case), case.claims
    assert len(a) == len(case.rings)
    for r, f in enumerate(a):
        assert f["max_scaled"] < 2.0**23, "the kernel's integer index and PCL's float one agree below 2^23 only"
        assert f["m"] != 1 and f["m"] <= lc.LFV_MAX - 2 * case.cr - 1 + (max(case.sizes()) > lc.LFV_MAX)
        if f["passthrough"]:   # (0 + -0.0) / 1 is +0.0 on the device, PCL copies: kept out of the cases
            assert not np.signbit(case.ring_candidates(r)[case.ring_candidates(r) == 0]).any()
    if cl.get("passthrough") is False:
        assert not any(f["passthrough"] for f in a)
    if "ring_len" in cl:
        assert all(n == cl["ring_len"] for n in case.sizes())
    if "ring_lens" in cl:
        assert case.sizes() == cl["ring_lens"]
    for key in ("m", "voxels", "passes"):
        if "per_ring_" + key in cl:
            assert [f[key] for f in a] == cl["per_ring_" + key], key
    if len(a) > 1:
        return
    f = a[0]
    for key in ("dims", "passthrough", "guards", "bits", "passes", "m", "voxels", "longest_run", "straddles", "heads_at", "ends_at",
                "per_wave", "negative"):
        if key in cl:
            assert f[key] == cl[key], (key, f[key])
    assert f["order_sensitive"] >= cl.get("min_order_sensitive", 0), f["order_sensitive"]
    assert f["on_faces"] >= cl.get("min_on_faces", 0), f["on_faces"]
    if "digits" in cl:
        assert len(f["digits"]) == len(cl["digits"])
        for got, want in zip(f["digits"], cl["digits"]):
            assert got[0] == want[0] and (want[1] is None or got[1] == want[1]), (got, want)


def test_the_set_reaches_every_path():
    per_ring = [f for c in CASES for f in _analysis(c)]
    live = [f for f in per_ring if f["m"] > 0]
    assert {f["passes"] for f in live if not f["passthrough"]} == {0, 1, 2, 3, 4}
    assert any(f["passthrough"] for f in live)
    assert {"dxdy", "dz", "dxdydz"} == {g for f in live for g in f["guards"]}
    assert {("dxdydz",), ("dxdy", "dxdydz"), ("dz", "dxdydz")} <= {f["guards"] for f in live}
    assert {f["per_wave"] for f in live} == {64, 128, 192, 256}
    assert {2, 1024, 1025, 2049, 3073, 4093} <= {f["m"] for f in live}
    assert any(f["m"] == 0 for f in per_ring)
    assert sum(f["order_sensitive"] for f in live) >= 200
    assert {1024, 2048, 3072} <= {s for f in live for s in f["straddles"]}
    assert any(f["longest_run"] > 1024 for f in live) and any(256 < f["longest_run"] <= 1024 for f in live)
    # odd pass counts end in the second key buffer and are copied back, even ones are not: both with more than one wave's share
    assert {1, 3} <= {f["passes"] for f in live if f["m"] > 1024} and {2, 4} <= {f["passes"] for f in live if f["m"] > 1024}


def test_mixed_batch_and_dispatch_shapes():
    mixed = lc.by_name("mixed batch", CASES)
    m = [f["m"] for f in _analysis(mixed)]
    assert max(mixed.sizes()) == lc.LFV_MAX and 0 in m and 2 in m and any(1000 <= v <= 1024 for v in m) and max(m) == 4085
    assert len({f["passes"] for f in _analysis(mixed) if f["m"]}) >= 3   # rings of different key widths side by side
    longer = EXTRA[2]
    assert max(longer.sizes()) == lc.LFV_MAX + 1 and longer.sizes()[1:] == mixed.sizes()[1:]
    a, b = EXTRA[:2]
    assert a.sizes() == [4096] and b.sizes() == [4097]
    fa, fb = _analysis(a)[0], _analysis(b)[0]
    # the extra pad point joins the first body point, which was alone in its voxel: same voxels, same means (2a / 2 == a)
    first = int(np.flatnonzero(fa["order"] == 0)[0])
    run = int(np.searchsorted(fa["run_start"], first, side="right") - 1)
    assert fa["run_end"][run] - fa["run_start"][run] == 1 and fb["voxels"] == fa["voxels"] and fb["m"] == fa["m"] + 1


def test_reuse_sequence_names_exist():
    for name in lc.REUSE_ORDER:
        assert lc.by_name(name, CASES).name == name
    sizes = [max(lc.by_name(n, CASES).sizes()) for n in lc.REUSE_ORDER]
    assert sizes[0] == 4096 and sizes[1] == 13 and sizes[-1] == 4096   # P * 24 > 64 KB, then a few hundred bytes, then large again


def test_dispatch_pair_has_one_less_flat_cloud(orc):
    (a, _), (b, _) = (lc.cached_reference(orc, c) for c in EXTRA[:2])
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@_by_name(CASES + EXTRA)
def test_premise_the_oracles_scan_registration_gives_the_reference(orc, case):
    """the huge threshold makes every region point a less-flat candidate and nothing a corner: the oracle's full extraction equals
    the per-ring voxel grid of the candidates byte for byte"""
    f = op.ScanRegistration(orc, **case.oracle_config()).process(case.cloud(), case.sizes())
    ref, off = lc.cached_reference(orc, case)
    assert f["less_flat"].shape == ref.shape and np.array_equal(f["less_flat"].view(np.uint32), ref.view(np.uint32))
    assert len(f["sharp"]) == 0 and len(f["less_sharp"]) == 0
    assert off[-1] == len(ref)


def test_the_kernels_specification_equals_the_oracle_and_wrong_models_do_not(orc):
    """teeth: the designed grid (integer index, stable sort, sums from 0 in input order, pass-through) equals the oracle on every
    case; each wrong model differs on at least one, and the cases written for it are among those"""
    def differs(case, **kw):
        got, (ref, _) = lc.model(case, **kw), lc.cached_reference(orc, case)
        return got.shape != ref.shape or not np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    for case in CASES + EXTRA:
        assert not differs(case), case.name
    caught = {wrong: [c.name for c in CASES if differs(c, **kw)]
              for wrong, kw in (("reversed sums", dict(reverse=True)), ("unstable sort", dict(unstable=True)),
                                ("no pass-through", dict(passthrough=False)))}
    for wrong, names in caught.items():
        print(f"{wrong}: caught by {names}")
    assert {"one voxel", "1 pass", "4 passes, dense runs", "head at 1023"} <= set(caught["reversed sums"])
    assert {"one voxel", "1 pass", "4 passes, dense runs"} <= set(caught["unstable sort"])
    assert set(caught["no pass-through"]) == {"2^31 voxels", "sheet", "tall"}
