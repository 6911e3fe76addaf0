"""CPU: every re-projection case (tests/reproject_cases.py) is what it claims to be; the float32 restatement
(tests/reproject_model.py) equals the oracle's transform_to_end / transform_to_start word for word where both are defined and agrees
with the float64 model within the measured bound; KAPPA is what the oracle's deviation from the float64 model measures; the header
and the binding agree, and the probe refuses bad arguments before it touches a device."""
import os

import numpy as np
import pytest

import oracle_py as op
import reproject_cases as rc
import reproject_model as rm
from conftest import ROOT

CASES = rc.all_cases()
BY_NAME = {c.name: c for c in CASES}
ids = lambda c: c.name


def of(cls):
    return [c for c in CASES if c.cls == cls]


def test_every_family_is_there():
    names = set(BY_NAME)
    assert len(names) == len(CASES)
    for kind in ("translation", "shift", "imu_rot"):
        assert {f"exact_{kind}_p0.1", f"exact_{kind}_p0.05"} <= names
    assert {f"exact_n{n}" for n in (0, 1, 63, 64, 65, 255, 256, 257, 4097)} <= names
    assert {f"exact_K{K}_ns{ns}" for K in (1, 2, 6, 64) for ns in (1, 2, 3) if ns <= K} <= names
    assert {f"order_descent_at_{i}" for i in (1, 63, 64, 65, 255, 256, 257, 4096)} <= names
    assert {f"order_ring_{r}" for r in (254, 255, 318, 319, 400)} <= names
    assert max(c.n for c in CASES) <= 70000
    assert [c.epoch for c in rc.epoch_sequence()] == [254, 255, 1]


@pytest.mark.parametrize("case", CASES + rc.epoch_sequence(), ids=ids)
def test_case_is_well_formed(case):
    off = case.off.astype(np.int64)
    assert off[0] == 0 and off[-1] == case.n and (np.diff(off) >= 0).all() and 1 <= case.ns <= case.K <= 4096
    assert 1 <= case.epoch <= 255 and 0 <= case.n_corner_all <= case.n
    assert np.isfinite(case.pts).all() and (case.pts[:, 3] >= 0).all() and (case.pts[:, 3] < 1024).all()
    assert case.params.dtype == rm.PARAMS and case.table_in.shape == (case.K, rm.RF_N) and case.bounds_in.shape == (case.K, 6)
    for P in case.params:
        frac = case.pts[:, 3] - np.trunc(case.pts[:, 3])
        assert (frac < P["scan_period"]).all(), "the time fraction stays below the scan period"
        for s, c in (("sT", "cT"), ("s_start", "c_start"), ("s_end", "c_end")):
            unit = P[s].astype(np.float64) ** 2 + P[c].astype(np.float64) ** 2
            assert (np.abs(unit - 1.0) <= 2.0 ** -23).all(), "sine / cosine words are a unit pair to 1 ulp"
        if case.cls != "general":
            assert (P["T"][:3] == 0).all() and (P["sT"] == 0).all() and (P["cT"] == 1).all()
    assert not (case.table_in >> 24 == case.epoch).any(), "the caller's fill never looks like an entry of this call"


@pytest.mark.parametrize("case", of("exact"), ids=ids)
def test_exact_case_holds_its_claim(case):
    cl = case.claims
    if cl.get("imu_zero"):
        for P in case.params:
            assert (P["s_start"] == 0).all() and (P["s_end"] == 0).all() and (P["c_start"] == 1).all() and (P["c_end"] == 1).all()
    if cl.get("fields"):
        w = case.pts[:, 3]
        frac = w - np.trunc(w)
        assert set(np.trunc(w).astype(int)) == {0, 1, 127, 254}
        for ring in (0, 1, 127, 254):
            f = frac[np.trunc(w) == ring]
            step = np.nextafter(np.float32(ring), np.float32(1e9)) - np.float32(ring)
            assert (f == 0).any() and (f == step).any() and (np.float32(0.1) - f.max()) <= 2 * max(step, np.float32(2.0 ** -27))
        u = case.pts[:, :3].view(np.uint32)
        assert (u == 0x80000000).any() and (u == 0).any() and np.abs(case.pts[:, :3]).max() == 300.0
    if cl.get("distinct_params"):
        out = [rm.to_end_f32(case.pts, P) for P in case.params]
        for a in range(case.ns):
            for b in range(a + 1, case.ns):
                assert np.abs(out[a][:, :3] - out[b][:, :3]).max(axis=1).min() > 1.0, "a neighbour's record moves every point by metres"
        assert (np.diff(case.off.astype(np.int64)) > 0).sum() >= min(case.K, 2 * case.ns) or case.K == 64
    if "passthrough" in cl:
        assert [c for c in range(case.K) if not case.params[c % case.ns]["enabled"]] == cl["passthrough"]
        a, b = case.off[1], case.off[2]
        assert b - a >= 2 and (case.pts[a:b, 3] != np.trunc(case.pts[a:b, 3])).any()


@pytest.mark.parametrize("case", of("order"), ids=ids)
def test_order_case_holds_its_claim(case):
    cl = case.claims
    w_out = rm.batch(rm.to_end_f32, case.pts, case.off, case.params)[:, 3]
    table, choices = rm.ring_table(w_out, case.off, case.epoch, case.table_in)
    stamped = [c for c in range(case.K) if table[c, rm.RF_N - 1] == case.epoch]
    assert stamped == cl["stamped"]
    if "descents" in cl:
        assert rm.descents(case.pts[:, 3], case.off) == cl["descents"], "exactly one descent, at the stated index"
        i = cl["descents"][0]
        assert int(case.pts[i - 1, 3]) - int(case.pts[i, 3]) == (1 if cl.get("by_one") else 2)
    elif not cl.get("multi_head"):
        assert rm.descents(case.pts[:, 3], case.off) == []
    if "rings" in cl:
        written = [r for r in range(rm.RF_N - 1) if table[0, r] != rc.FILL]
        assert written == cl["rings"]
    if cl.get("multi_head"):
        assert len(choices) >= 2
    elif "descents" not in cl:
        assert not choices, "an ordered cloud has one run head per ring"
    # untouched words keep the fill; written ones carry the epoch and an index inside the cloud
    wrote = table != case.table_in
    assert ((table[:, :-1][wrote[:, :-1]] >> 24) == case.epoch).all()
    lens = np.diff(case.off.astype(np.int64))
    for c in range(case.K):
        assert ((table[c, :-1][wrote[c, :-1]] & 0xffffff) < max(lens[c], 1)).all()
    if case.name.startswith("order_drop_across"):
        nz = [c for c in range(case.K) if lens[c]]
        a, b = case.off[nz[1]] - 1, case.off[nz[1]]
        assert int(case.pts[a, 3]) > int(case.pts[b, 3])
    if case.name == "order_one_violating_among_six":
        assert (wrote[:, -1] == [False, False, False, True, False, False]).all()


def test_epoch_sequence_keeps_what_later_calls_do_not_touch():
    seq = rc.epoch_sequence()
    table = np.full((2, rm.RF_N), rc.FILL, np.uint32)
    for case in seq:
        w_out = rm.batch(rm.to_end_f32, case.pts, case.off, case.params)[:, 3]
        table, choices = rm.ring_table(w_out, case.off, case.epoch, table)
        assert set(k for k in choices if k[0] == 1) == set()
    assert table[0, rm.RF_N - 1] == 254 and table[1, rm.RF_N - 1] == rc.FILL      # unordered at 254, ordered afterwards: the stamp stays
    assert table[0, 10] >> 24 == 254 and table[0, 15] >> 24 == 255 and table[0, 20] >> 24 == 1
    assert table[1, 0] >> 24 == 254 and table[1, 12] >> 24 == 255 and table[1, 5] >> 24 == 1


@pytest.mark.parametrize("case", of("bounds"), ids=ids)
def test_bounds_case_holds_its_claim(case):
    out = rm.batch(rm.to_end_f32, case.pts, case.off, case.params)
    bb = rm.bounds(out, case.off, case.bounds_in)
    lens = np.diff(case.off.astype(np.int64))
    for c in range(case.K):
        if lens[c] == 0:
            assert (bb[c] == case.bounds_in[c]).all()
        else:
            lo, hi = rm.dec_f32(bb[c, :3]), rm.dec_f32(bb[c, 3:])
            assert (lo <= hi).all() or (case.bounds_in[c] != rm.RESET).any()
    if case.claims.get("mixed"):
        assert any(o % 64 for o in case.off[1:-1])
        assert rm.dec_f32(bb[0, 0]) == -1000.0 and rm.dec_f32(bb[2, 5]) > -1000.0
    if case.claims.get("extremes"):
        e = rm.enc_f32(out[:, :3])
        assert e[:, 0].argmax() == 0 and e[:, 0].argmin() == case.n - 1 and e[:, 1].argmax() == 63 and e[:, 1].argmin() == 64
        assert e[:, 2].argmax() == 255 and e[:, 2].argmin() == 256


def test_encoding_round_trips_and_orders():
    v = np.array([-np.inf, -300.0, -1e-45, -0.0, 0.0, 1e-45, 300.0, np.inf], np.float32)
    e = rm.enc_f32(v)
    assert (np.diff(e.astype(np.int64)) > 0).all() and np.array_equal(rm.dec_f32(e).view(np.uint32), v.view(np.uint32))


# ---- the models against each other and against the oracle ------------------------------------------------------------------
def _oracle(orc, case, which):
    """the oracle per cloud at the cloud's record: set_transform + update_imu with zero velocity (the pose the too-few-points guard
    leaves untouched), then transform_to_end of the cloud / transform_to_start of every point.  IMU angles enter as angles, so this
    needs records made from angles (rm.make_params) or zero IMU rotations."""
    out = np.zeros((case.n, 4), np.float32)
    for c in range(case.K):
        a, b = int(case.off[c]), int(case.off[c + 1])
        P = case.params[c % case.ns]
        od = op.LaserOdometry(orc, scanPeriod=float(P["scan_period"]))
        od.set_transform(P["T"])
        if case.imu_angles is None:
            assert (P["s_start"] == 0).all() and (P["s_end"] == 0).all() and (P["c_start"] == 1).all() and (P["c_end"] == 1).all()
        ang = np.zeros(6, np.float32) if case.imu_angles is None else case.imu_angles[c % case.ns]
        t12 = np.concatenate([ang, P["shift"], np.zeros(3, np.float32)]).astype(np.float32)
        od.update_imu(t12)
        if b > a:
            out[a:b] = od.to_end(case.pts[a:b]) if which == "end" else od.to_start(case.pts[a:b])
    return out


ORACLE_EXACT = [c for c in of("exact") + of("order") + of("bounds") if all((P["s_start"] == 0).all() and (P["s_end"] == 0).all() for P in c.params)]


@pytest.mark.parametrize("case", ORACLE_EXACT, ids=ids)
def test_f32_model_equals_the_oracle_word_for_word(orc, case):
    for which, fn in (("end", rm.to_end_f32), ("start", rm.to_start_f32)):
        m = rm.batch(fn, case.pts, case.off, case.params, passthrough=False)
        o = _oracle(orc, case, which)
        assert np.array_equal(m.view(np.uint32), o.view(np.uint32)), which


def test_the_oracle_comparison_covers_the_edge_fields():
    names = {c.name for c in ORACLE_EXACT}
    assert {"exact_fields_trans_shift", "exact_translation_p0.05", "exact_shift_p0.1", "exact_n4097"} <= names and len(names) >= 40


@pytest.mark.parametrize("case", of("exact") + of("order") + of("bounds"), ids=ids)
def test_f32_model_stays_within_the_bound_of_the_f64_model(case):
    for f32, f64 in ((rm.to_end_f32, rm.to_end_f64), (rm.to_start_f32, rm.to_start_f64)):
        for c in range(case.K):
            a, b = int(case.off[c]), int(case.off[c + 1])
            P = case.params[c % case.ns]
            err = np.abs(f32(case.pts[a:b], P).astype(np.float64) - f64(case.pts[a:b], P))
            assert (err[:, :3] <= rm.bound(case.pts[a:b], P)[:, None]).all() and (err[:, 3] == 0).all()


def oracle_ratio(orc, case):
    """the oracle's worst deviation from the f64 model in units of 2^-24 * scale, over transform_to_end and transform_to_start"""
    worst = 0.0
    for which, f64 in (("end", rm.to_end_f64), ("start", rm.to_start_f64)):
        o = _oracle(orc, case, which).astype(np.float64)
        for c in range(case.K):
            a, b = int(case.off[c]), int(case.off[c + 1])
            if b > a:
                P = case.params[c % case.ns]
                err = np.abs(o[a:b, :3] - f64(case.pts[a:b], P)[:, :3]).max(axis=1)
                worst = max(worst, float((err / (2.0 ** -24 * rm.scale(case.pts[a:b], P))).max()))
    return worst


def test_kappa_is_what_the_oracle_measures(orc):
    """KAPPA covers the oracle's deviation from the f64 model on every general-class case, and is not loose: the measured worst
    ratio, rounded up to two digits"""
    worst = max(oracle_ratio(orc, c) for c in of("general"))
    print(f"oracle worst ratio {worst:.4f}, KAPPA {rm.KAPPA}, kernel bound {rm.DEVICE_FACTOR} x")
    assert worst <= rm.KAPPA <= 1.15 * worst


def test_general_records_are_made_from_float32_angles():
    """what lets the oracle (which takes angles) and the probe (which takes words) be driven alike: a record's words are the
    float32 nearest to the true sine / cosine of the float32 angles the case keeps beside it"""
    for case in of("general"):
        for P, ang in zip(case.params, case.imu_angles):
            for s, c, a in (("sT", "cT", P["T"][:3]), ("s_start", "c_start", ang[:3]), ("s_end", "c_end", ang[3:])):
                assert a.dtype == np.float32
                assert np.array_equal(np.sin(a.astype(np.float64)).astype(np.float32), P[s]) and np.array_equal(np.cos(a.astype(np.float64)).astype(np.float32), P[c])
            assert np.abs(P["T"][:3]).max() <= 0.3 and np.abs(P["T"][3:]).max() <= 3 and np.abs(P["shift"]).max() <= 2
        assert np.linalg.norm(case.pts[:, :3], axis=1).max() <= 120.0 and case.pts[:, 3].max() < 128


# ---- the header, the binding, the refusals ---------------------------------------------------------------------------------
def test_header_and_binding_agree():
    from loam_velodyne_amd import loamx
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    assert "int loamx_reproject_probe(" in hdr and "#define LOAMX_ABI_VERSION 6" in hdr
    for name, val in (("BATCH", 0), ("FUSED", 1), ("SINGLE", 2), ("COPY", 3), ("GATHER", 4), ("TO_START", 5), ("NO_RING_TABLE", 8), ("NO_BOUNDS", 16)):
        assert f"#define LOAMX_REPROJECT_{name} {val}u" in hdr and getattr(loamx, f"REPROJECT_{name}") == val
    assert loamx.REPROJECT_PARAMS == rm.PARAMS and rm.PARAMS.itemsize == 29 * 4 and loamx.REPROJECT_RF_N == rm.RF_N
    body = hdr[hdr.index("typedef struct loamx_reproject_params {"):hdr.index("} loamx_reproject_params;")]
    fields = [f for f in ("T[6]", "sT[3], cT[3]", "shift[3]", "s_start[3], c_start[3]", "s_end[3], c_end[3]", "scan_period", "enabled")]
    assert [body.index(f) for f in fields] == sorted(body.index(f) for f in fields)
    src = open(os.path.join(ROOT, "loam_velodyne_amd", "csrc", "api_probe.hip")).read()
    assert "static_assert(sizeof(ToEndParams) == sizeof(loamx_reproject_params)" in src
    assert hasattr(loamx.lib(), "loamx_reproject_probe")


def refusals():
    """(name, keyword changes) that loamx_reproject_probe must answer with LOAMX_E_INVALID before it touches a device"""
    nan = np.zeros((4, 4), np.float32); nan[2, 1] = np.nan
    inf = np.zeros((4, 4), np.float32); inf[0, 0] = np.inf
    wneg = np.zeros((4, 4), np.float32); wneg[1, 3] = -0.5
    wbig = np.zeros((4, 4), np.float32); wbig[3, 3] = 1024.0
    wnan = np.zeros((4, 4), np.float32); wnan[3, 3] = np.nan
    return [("off_not_from_0", dict(off=[1, 4])), ("off_not_to_n", dict(off=[0, 3])), ("off_decreasing", dict(off=[0, 3, 2, 4])),
            ("ns_0", dict(params=0)), ("ns_above_K", dict(params=2)), ("epoch_0", dict(epoch=0)), ("epoch_256", dict(epoch=256)),
            ("nan_coordinate", dict(points=nan)), ("inf_coordinate", dict(points=inf)), ("w_negative", dict(points=wneg)), ("w_1024", dict(points=wbig)),
            ("w_nan", dict(points=wnan)), ("unknown_flag", dict(flags=32)), ("unknown_variant", dict(flags=6)), ("n_corner_all_beyond_n", dict(n_corner_all=5))]


def call_refused(loamx, kw):
    args = dict(points=np.zeros((4, 4), np.float32), off=[0, 4], params=1, epoch=1, n_corner_all=0, flags=0)
    args.update(kw)
    args["params"] = np.array([rm.identity_params()] * args["params"], rm.PARAMS) if args["params"] else np.zeros(0, rm.PARAMS)
    with pytest.raises(loamx.LoamxError) as e:
        loamx.reproject_probe(**args)
    return e.value.code


@pytest.mark.parametrize("name,kw", refusals(), ids=[r[0] for r in refusals()])
def test_refused_before_a_device_is_touched(name, kw):
    from loam_velodyne_amd import loamx
    assert call_refused(loamx, kw) == loamx.E_INVALID


def test_null_pointers_and_K_range_are_refused():
    import ctypes as C
    from loam_velodyne_amd import loamx
    L = loamx.lib()
    p = np.zeros((4, 4), np.float32); off = np.array([0, 4], np.uint32); par = np.array([rm.identity_params()], rm.PARAMS)
    out = np.zeros((4, 4), np.float32); rf = np.zeros(rm.RF_N, np.uint32); bb = np.zeros(6, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    good = [ptr(p), C.c_uint32(4), ptr(off), C.c_uint32(1), ptr(par), C.c_uint32(1), C.c_uint32(1), C.c_uint32(0), C.c_uint32(0), ptr(out), ptr(rf), ptr(bb)]
    for k in (0, 2, 4, 9, 10, 11):
        args = list(good)
        args[k] = None
        assert L.loamx_reproject_probe(*args) == loamx.E_INVALID, k
    for K in (0, 4097):
        args = list(good)
        args[3] = C.c_uint32(K)
        assert L.loamx_reproject_probe(*args) == loamx.E_INVALID, K
