"""CPU: every order case of the bucketed voxel grid (tests/voxbucket_order_cases.py) is the edge it claims to be, by the model
(tests/voxbucket_model.py), and for every case that does not give up the model's result equals pcl::VoxelGrid per segment (the
oracle, on the model's stack) word for word — the way tests/test_voxbucket_cases_cpu.py holds the cases of voxbucket_cases.py."""
import numpy as np
import pytest

import voxbucket_model as vm
import voxbucket_order_cases as oc
import voxel_cases as vc

SUBSET_CLAIMS = {"counts": "cnt", "runs": "runs", "has_passes": "passes"}


def test_every_case_is_there():
    for name in ("sum_order", "interleaved", "sparse_chunks", "sparse_large", "chunk_edges", "exactly_full", "share_edges", "refused_between"):
        assert name in oc.BUILDERS
    for k in (8, 9, 16, 17, 24, 25):
        assert f"key_bits_{k}" in oc.BUILDERS
    assert len(oc.get("sum_order").pts) >= 3 * 256 and len(oc.get("sparse_chunks").pts) >= 8 * 256


@pytest.mark.parametrize("name", oc.NAMES)
def test_case_is_what_it_claims(name):
    case = oc.get(name)
    R = case.model()
    f = oc.facts(case, R)
    assert R.gave_up == bool(case.claims["reasons"])
    for key, want in case.claims.items():
        if key in SUBSET_CLAIMS:
            assert set(want) <= set(f[SUBSET_CLAIMS[key]]), key
        elif key in ("range_without", "voxels_of"):
            for b, v in want.items():
                assert f[key].get(b) == v, (key, b, f[key].get(b))
        else:
            assert f[key] == want, (key, f[key])
    if not R.gave_up:
        assert int(R.cnt.max()) <= vm.VB_CAP and int(R.cnt.sum()) == case.n and int(R.out_off[-1]) == len(R.out)


def test_the_pass_counts_of_the_voxel_bits_are_covered():
    """one, two, three and four passes on the voxel bits alone, on both sides of every edge"""
    got = {k: -(-k // 8) for name in oc.NAMES if name.startswith("key_bits_") for k in oc.get(name).claims["key_bits"]}
    assert got == {8: 1, 9: 2, 16: 2, 17: 3, 24: 3, 25: 4}


def test_sum_order_is_the_sequential_sum():
    """the expected mean, spelled out: float32 sums from 0 in input order"""
    case = oc.get("sum_order")
    acc = np.float32(0.0)
    for w in (1e8, 1.0, -1e8, 0.5):
        acc = np.float32(acc + np.float32(w))
    assert acc == np.float32(0.5)
    R = case.model()
    row = R.out[R.out[:, 0] >= 20.0]
    assert len(row) == 1 and row[0, 3] == acc / np.float32(4.0)
    # and in the reverse order it is another number
    rev = np.float32(0.0)
    for w in (0.5, -1e8, 1.0, 1e8):
        rev = np.float32(rev + np.float32(w))
    assert rev != acc


@pytest.mark.parametrize("name", oc.NAMES)
def test_the_model_equals_the_oracle(orc, name):
    case = oc.get(name)
    R = case.model()
    if R.gave_up:
        assert R.reasons == case.claims["reasons"] and not hasattr(R, "out")
        return
    ref, ref_off = vc.reference(orc, case.voxel_case(R.stack))
    assert np.array_equal(R.out_off, ref_off)
    assert R.out.shape == ref.shape and np.array_equal(R.out.view(np.uint32), ref.view(np.uint32))
