"""CPU: every generated case of the bucketed voxel grid (tests/voxbucket_cases.py) is the edge it claims to be, by the model
(tests/voxbucket_model.py): bucket counts, position bits, sort passes, workgroups whose buckets meet in the slot table, segment
boundaries inside a workgroup, run positions, the reason set of every give-up — and "no bucket above VB_CAP" for every large case that
is to succeed.  For every case that does not give up, the model's result equals pcl::VoxelGrid per segment (the oracle, on the model's
stack) word for word, and does not change when the points arrive in another order."""
import numpy as np
import pytest

import voxbucket_cases as bc
import voxbucket_model as vm
import voxel_cases as vc

SUBSET_CLAIMS = {"counts": "cnt", "runs": "runs", "has_passes": "passes"}


def test_every_family_is_there():
    for n in (1, 2, 511, 512, 513, 2047, 2048, 2049, 4096, 4097):
        assert f"ns_{n}" in bc.BUILDERS
    for n in (131072, 131073, 524289, 1048576, 1048577):
        assert f"large_{n}" in bc.BUILDERS
    for k in range(1, 8):
        assert f"passes_{k}" in bc.BUILDERS
    for k in (1, 2, 3, 511, 512, 513, 4096):
        assert f"nseg_{k}" in bc.BUILDERS
    for name in bc.REUSE:
        assert name in bc.BUILDERS
    assert [bool(bc.get(k).claims["reasons"]) for k in bc.REUSE] == [False, False, True, False, False, False]
    flags = {bc.get(k).flags for k in ("ragged", "ragged_concatenated", "nseg_513", "nseg_512")}
    assert flags == {0, bc.SRC_POINTERS}


@pytest.mark.parametrize("name", bc.NAMES)
def test_case_is_what_it_claims(name):
    case = bc.get(name)
    R = case.model()
    f = bc.facts(case, R)
    assert R.gave_up == bool(case.claims["reasons"])
    for key, want in case.claims.items():
        if key in SUBSET_CLAIMS:
            assert set(want) <= set(f[SUBSET_CLAIMS[key]]), key
        elif key == "one_voxel":
            assert want in f["one_voxel"], key
        else:
            assert f[key] == want, key
    if not R.gave_up:
        assert int(R.cnt.max()) <= vm.VB_CAP, "no bucket above capacity"
        assert int(R.cnt.sum()) == case.n and int(R.out_off[-1]) == len(R.out)
    # the plan words hang together
    assert np.array_equal(R.segs["bucket0"], np.concatenate([[0], np.cumsum(np.maximum(1, -(-np.diff(case.seg_off.astype(np.int64)) // vm.VB_T)))[:-1]]))
    for s in np.flatnonzero(R.segs["nbuckets"]):
        lo = R.lo[int(R.segs["bucket0"][s]):int(R.segs["bucket0"][s] + R.segs["nbuckets"][s])]
        assert lo[0] == 0 and np.all(lo[1:] >= lo[:-1])


def test_every_pass_count_and_both_searches_are_covered():
    passes, lds, glob = set(), False, False
    for name in bc.NAMES:
        case = bc.get(name)
        if case.claims["reasons"]:
            continue
        R = case.model()
        passes |= {int(-(-b // 8)) for b in R.bucket_bits if b}
        k = R.segs["nbuckets"]
        lds |= bool(((k > 1) & (k <= 64)).any())
        glob |= bool((k > 64).any())
    assert passes == {1, 2, 3, 4, 5, 6, 7} and lds and glob
    assert bc.get("large_131072").model().segs["nbuckets"][0] == 64 and bc.get("large_131073").model().segs["nbuckets"][0] == 65


@pytest.mark.parametrize("name", bc.NAMES)
def test_the_model_equals_the_oracle_in_any_arrival_order(orc, name):
    case = bc.get(name)
    R = case.model()
    if R.gave_up:
        assert R.reasons == case.claims["reasons"] and not hasattr(R, "out")
        return
    ref, ref_off = vc.reference(orc, case.voxel_case(R.stack))
    assert np.array_equal(R.out_off, ref_off)
    assert R.out.shape == ref.shape and np.array_equal(R.out.view(np.uint32), ref.view(np.uint32))
    other = vm.run(case.pts, case.seg_off, case.poses, case.leaf_even, case.leaf_odd, arrival=np.random.default_rng(5).permutation(case.n))
    assert np.array_equal(other.out_off, R.out_off) and np.array_equal(other.out.view(np.uint32), R.out.view(np.uint32))
    for k in ("lo", "cnt", "segs", "stack"):
        assert np.array_equal(getattr(other, k), getattr(R, k)), k


def test_round_trip_words():
    """identity: exact but for the sign of a zero; the pose words are those of pose_set_angles (sine / cosine rounded from double)"""
    c = bc.get("faces_identity")
    R = c.model()
    assert np.array_equal(R.stack, c.pts) and not np.array_equal(R.stack.view(np.uint32), c.pts.view(np.uint32))
    w = vm.pose_words(0.25, -0.5, 1.0, 1, 2, 3)
    assert w.dtype == np.float32 and w[6] == np.float32(np.sin(0.25)) and w[11] == np.float32(np.cos(1.0)) and w[8] == np.float32(np.sin(-0.5))
    # a rotation about one axis only, against the same arithmetic written out in float32 scalars
    p = np.array([[1.5, -2.25, 0.75, 9.0]], np.float32)
    T = vm.pose_words(0, 0, 0.3, 10, 20, 30)
    c_, s_ = T[11], T[10]
    x = np.float32(np.float32(c_ * p[0, 0]) - np.float32(s_ * p[0, 1]))
    y = np.float32(np.float32(s_ * p[0, 0]) + np.float32(c_ * p[0, 1]))
    x, y, z = np.float32(np.float32(x + T[3]) - T[3]), np.float32(np.float32(y + T[4]) - T[4]), np.float32(np.float32(p[0, 2] + T[5]) - T[5])
    x2 = np.float32(np.float32(c_ * x) - np.float32(np.float32(-s_) * y))
    y2 = np.float32(np.float32(np.float32(-s_) * x) + np.float32(c_ * y))
    got = vm.round_trip(p, T[None])
    assert np.array_equal(got[0], np.array([x2, y2, z, 9.0], np.float32))


def test_the_probe_is_declared_exported_and_refuses_before_it_touches_a_device():
    import os
    from loam_velodyne_amd import loamx
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "loamx.h")).read()
    assert "int loamx_voxbucket_probe(" in hdr and "#define LOAMX_VOXBUCKET_SRC_POINTERS 1u" in hdr and "#define LOAMX_ABI_VERSION 6" in hdr
    assert hasattr(loamx.lib(), "loamx_voxbucket_probe") and loamx.VOXBUCKET_SRC_POINTERS == bc.SRC_POINTERS
    assert loamx.VOXBUCKET_SEG.itemsize == 16 and loamx.VOXBUCKET_SEG.names == vm.SEG_DTYPE.names
    p = np.zeros((4, 4), np.float32)
    for off, leaf in (([0, 3], 0.5), ([0, 4], 0.0), ([0, 3, 2, 4], 0.5)):
        with pytest.raises(loamx.LoamxError) as e:
            loamx.voxbucket_probe(p, off, np.tile(vm.IDENTITY, ((len(off)) // 2, 1)), leaf)
        assert e.value.code == loamx.E_INVALID
