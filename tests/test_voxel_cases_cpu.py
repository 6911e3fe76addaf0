"""CPU: every generated voxel-grid case (tests/voxel_cases.py) is what it claims to be — recomputed in numpy int64 from
floor(p * (1/leaf)) in float32, as the kernels derive it: the number of key bits, which segments PCL passes through unfiltered, which
runs cross which tile ends in sorted order; and every case stays where the kernels' integer voxel index and PCL's float one agree
(axis extents <= 2^24 voxels, |p / leaf| < 2^30).  Plus the reference's bookkeeping against a plain per-segment loop."""
import numpy as np
import pytest

import voxel_cases as vc

CASES = vc.all_cases()


def test_every_family_is_there():
    names = [c.name for c in CASES]
    for B in vc.KEY_BITS:
        assert f"bits{B}_contiguous" in names and all(f"bits{B}_ids_nseg{k}" in names for k in vc.KEY_NSEG)
    for n in vc.TILE_EDGE_N:
        assert f"tile_single_n{n}" in names
    for k in vc.SEGMENT_NSEG:
        assert f"seg{k}_full_contiguous" in names and f"seg{k}_full_ids_interleaved" in names and f"seg{k}_full_ids_grouped" in names
        assert k == 1 or f"seg{k}_empties_contiguous" in names
    assert vc.dims_for_bits(31) == (2**11, 2**10, 2**10 - 1)
    assert sorted({c.n for c in CASES})[0] == 0 and max(c.n for c in CASES) <= 20000


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_is_what_it_claims(case):
    a = vc.analyse(case)
    assert a["B"] == case.claims["B"], "key bits of the largest linear voxel index among the filtered segments"
    assert a["passthrough"] == sorted(case.claims["passthrough"]), "segments of more than INT_MAX voxels"
    assert a["max_extent"] <= 2**24 and a["max_scaled"] < 2.0**30
    for key in ("cross", "ends_on_tile", "starts_on_tile", "head_last_of_tile"):
        if key in case.claims:
            assert a["general"][key] == case.claims[key], key
            if case.seg_kernel:
                assert a["seg"][key] == case.claims[key], key + " (segment-relative tiles)"
    assert 1 <= a["passes_general"] <= 6 and 1 <= a["passes_seg"] <= 4


def test_key_widths_cross_every_pass_count():
    """the general kernel sorts B + bits(nseg) bits in 8-bit digits (1..6 passes), the segmented one B bits in 9-bit digits (1..4)"""
    gen, seg = set(), set()
    for B in vc.KEY_BITS:
        for c in vc.key_width_cases(B):
            a = vc.analyse(c)
            gen.add(a["passes_general"])
            if c.seg_kernel:
                seg.add(a["passes_seg"])
    assert gen == {1, 2, 3, 4, 5, 6} and seg == {1, 2, 3, 4}


def test_empty_segments_are_where_the_family_says():
    for nseg in vc.SEGMENT_NSEG[3:]:
        c = [c for c in vc.segment_cases(nseg) if c.name == f"seg{nseg}_empties_contiguous"][0]
        ln = np.diff(c.seg_off.astype(np.int64))
        mid = nseg // 2
        assert ln[0] == 0 and ln[-1] == 0 and ln[mid // 2] == 0 and not ln[mid:mid + 3].any() and ln[1] > 0 and ln[mid + 3] > 0
        ci = [c for c in vc.segment_cases(nseg) if c.name == f"seg{nseg}_empties_ids_interleaved"][0]
        assert np.array_equal(np.flatnonzero(np.bincount(ci.seg_ids, minlength=nseg) == 0), np.flatnonzero(ln == 0))
        # interleaved: every wave of 64 consecutive points holds more than one segment
        assert all(len(set(ci.seg_ids[i:i + 64])) > 1 for i in range(0, ci.n - 64, 64))


def test_run_sums_depend_on_the_order():
    """the 5000-point voxel: summing its points in another order gives another float — a kernel that walked the run out of order would show"""
    c = [c for c in CASES if c.name == "run_5000_over_three_tiles"][0]
    vx = np.floor(c.pts[:, 0]).astype(int)
    run = c.pts[vx == np.argmax(np.bincount(vx))]
    assert len(run) == 5000

    def fsum(a):
        s = np.float32(0)
        for v in a:
            s = np.float32(s + v)
        return s
    for col in (0, 1, 3):
        assert fsum(run[:, col]) != fsum(run[::-1, col])


def test_reference_bookkeeping(orc):
    """reference(): per segment, the valid points in input order through the oracle's voxel grid with the segment's leaf"""
    for name in ("faces_dyadic_even_odd_ids", "mask_mixed_ids", "pass_between_ordinary_masked_ids", "mask_all_invalid_contiguous", "mask_n0_contiguous"):
        c = [c for c in CASES if c.name == name][0]
        out, off = vc.reference(orc, c)
        seg, ok = c.seg_of_point(), c.valid_mask()
        assert len(off) == c.nseg + 1 and off[0] == 0 and off[-1] == len(out)
        for s in range(c.nseg):
            want = orc.voxel_grid(c.pts[ok & (seg == s)], c.leaf_odd if s & 1 else c.leaf_even) if (ok & (seg == s)).any() else np.zeros((0, 4), np.float32)
            assert np.array_equal(out[off[s]:off[s + 1]].view(np.uint32), want.view(np.uint32)), (name, s)
        if name.startswith("pass_between"):   # the pass-through segment comes back as its valid input, in input order
            m = ok & (seg == 1)
            assert np.array_equal(out[off[1]:off[2]].view(np.uint32), c.pts[m].view(np.uint32))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_kernels_specification_equals_the_oracle(orc, case):
    """integer voxel index, stable sort, sums from 0 in input order, own keys in a pass-through segment — modelled in numpy — give the
    oracle's clouds word for word on every case: a mismatch on the device is then the kernels' implementation, not their design"""
    out, off = vc.model(case)
    ref, ref_off = vc.reference(orc, case)
    assert np.array_equal(off, ref_off)
    assert out.shape == ref.shape and np.array_equal(out.view(np.uint32), ref.view(np.uint32))
