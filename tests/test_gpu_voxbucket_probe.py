"""GPU: the bucketed voxel grid on its own (csrc/voxbucket.hip: k_vb_plan, k_vb_stack, k_vb_reduce through loamx_voxbucket_probe) at
the shapes where its kernels go wrong — bit for bit, no tolerance: every word the run leaves is specified.

A case that does not give up: the stack equals the model's (tests/voxbucket_model.py: the float32 round trip, one rounding per
operation), out / out_off equal pcl::VoxelGrid per segment as the oracle restates it ON that stack, the plan words — splitters, VbSeg
records, per-bucket counts — equal the model's, and the status says so.  A give-up case: the fail word is up, the reason mask is a
non-empty subset of the reasons the model finds (the set itself where it has one member), out_off is all zero, and the stack is still
the model's wherever the input was finite.  tests/voxbucket_cases.py builds the cases, tests/test_voxbucket_cases_cpu.py proves each
one is the edge it claims to be.

Regression kept here: test_pass_through.  A give-up raised inside k_vb_reduce (reason 2 by the last bucket at its end, reason 3) used
to leave out_off as a run that succeeded would — [0, 478] for pass_through_single; the bucket that arrives last now zeroes it.

Which case catches which break of the kernels (the searches, the fill and the mean were broken one at a time and run once on an
MI355X: exactly the cases listed failed; the other two breaks leave slot words that k_vb_reduce would read uninitialised, so they are
argued from the cases' proven claims, not run):
  `<=` -> `<` in the LDS search      cnt of ns_2049, ns_4096, ns_4097, large_131072, straddle_inside_workgroup, straddle_at_256, bucket_counts,
                                     one_voxel_4096, empties_lead_mid_trail, all_empty_but_one, ragged, ragged_concatenated: a key equal to a
                                     splitter changes bucket; the voxel means do not move — which is why the plan words are compared
  `<=` -> `<` in the global search   cnt of large_131073, large_524289, large_1048576, passes_7, straddle_inside_workgroup (segment 1 is not
                                     the workgroup's lead), test_reuse_of_the_object
  s_lo shortened to 32               with its fill (`threadIdx.x < 32`): large_131072, 64 splitters in LDS.  The declaration alone changes no
                                     instruction: s_lo is the last LDS variable and its upper half falls into the allocation's rounding
  a mean started from its first point  zero_sign (0 + -0.0 is +0.0)
  no `direct` branch                 large_524289, collide_alternating_empty: a workgroup there touches two buckets equal mod 256 (claim
                                     `collide`), whose slots and counts the table would merge
  cnt not reset by the plan          every call but the process's first; test_reuse_of_the_object by name (counts and slots carry over)
"""
import numpy as np
import pytest

import voxbucket_cases as bc
import voxel_cases as vc
from loam_velodyne_amd import loamx

pytestmark = pytest.mark.gpu

_REF = {}


def _reference(orc, case):
    """pcl::VoxelGrid per segment on the model's stack — computed once per case, shared, never written to"""
    if case.name not in _REF:
        _REF[case.name] = vc.reference(orc, case.voxel_case(case.model().stack))
    return _REF[case.name]


def _probe(case, flags=None):
    return loamx.voxbucket_probe(case.pts, case.seg_off, case.poses, case.leaf_even, case.leaf_odd, flags=case.flags if flags is None else flags)


def _words_equal(where, what, got, want):
    a, b = np.ascontiguousarray(got).view(np.uint32).reshape(len(got), -1), np.ascontiguousarray(want).view(np.uint32).reshape(len(want), -1)
    assert a.shape == b.shape, f"{where}: {what} has shape {a.shape}, expected {b.shape}"
    if not np.array_equal(a, b):
        r = int(np.flatnonzero((a != b).any(axis=1))[0])
        raise AssertionError(f"{where}: {what}: {int((a != b).any(axis=1).sum())} rows differ, first row {r}: {got[r]} != {want[r]}")


def check(orc, case, got, where=None):
    where = where or case.name
    R = case.model()
    assert got["buckets"] == R.buckets, f"{where}: last_buckets {got['buckets']} != {R.buckets}"
    if R.gave_up:
        assert got["gave_up"] == 1, f"{where}: the run did not give up (model: reasons {sorted(R.reasons)})"
        why = {r for r in range(32) if got["why"] >> r & 1}
        assert why and why <= R.reasons, f"{where}: reason mask {sorted(why)}, model {sorted(R.reasons)}"
        if len(R.reasons) == 1:
            assert why == R.reasons, where
        assert not got["out_off"].any(), f"{where}: out_off after a give-up: {got['out_off'][:8]} ..."
        finite = np.isfinite(case.pts[:, :3]).all(axis=1)
        _words_equal(where, "stack (finite input)", got["stack"][finite], R.stack[finite])
        return
    assert got["gave_up"] == 0, f"{where}: gave up, reason mask {got['why']:#x}"
    assert got["why"] == 0, where
    _words_equal(where, "stack", got["stack"], R.stack)
    _words_equal(where, "VbSeg records", got["segs"].view(np.uint32).reshape(-1, 4), R.segs.view(np.uint32).reshape(-1, 4))
    _words_equal(where, "splitters lo", got["lo"], R.lo)
    _words_equal(where, "cnt", got["cnt"], R.cnt)
    ref, ref_off = _reference(orc, case)
    off, out = got["out_off"], got["out"]
    if not np.array_equal(off, ref_off):
        s = int(np.flatnonzero(off != ref_off)[0])
        raise AssertionError(f"{where}: out_off differs first at [{s}]: {off[s]} != {ref_off[s]} (total {off[-1]} != {ref_off[-1]})")
    assert out.shape == ref.shape, where
    a, b = out.view(np.uint32), ref.view(np.uint32)
    if not np.array_equal(a, b):
        r = int(np.flatnonzero((a != b).any(axis=1))[0])
        s = int(np.searchsorted(ref_off, r, side="right") - 1)
        raise AssertionError(f"{where}: {int((a != b).any(axis=1).sum())} rows differ, first row {r} (segment {s}, its voxel {r - int(ref_off[s])}): "
                             f"{out[r]} != {ref[r]}")


def _family(prefix):
    return pytest.mark.parametrize("name", [k for k in bc.NAMES if k.startswith(prefix)])


@_family("ns_")
def test_segment_sizes(orc, name):
    check(orc, bc.get(name), _probe(bc.get(name)))


@_family("large_")
def test_large_segments(orc, name):
    """64 against 65 buckets (LDS against global splitters), 257 (slot-table collisions), 512 (look-back over hundreds), 513 (reason 1)"""
    check(orc, bc.get(name), _probe(bc.get(name)))


@pytest.mark.parametrize("name", ["collide_alternating_empty", "straddle_inside_workgroup", "straddle_at_256"])
def test_slot_table_and_lead_segment(orc, name):
    check(orc, bc.get(name), _probe(bc.get(name)))


@pytest.mark.parametrize("name", ["bucket_counts", "one_voxel_4096", "one_voxel_4097", "run_edges"])
def test_bucket_sizes_and_runs(orc, name):
    check(orc, bc.get(name), _probe(bc.get(name)))


@_family("passes_")
def test_sort_passes(orc, name):
    check(orc, bc.get(name), _probe(bc.get(name)))


@pytest.mark.parametrize("name", [k for k in bc.NAMES if k.startswith("nseg_")] + ["empties_lead_mid_trail", "all_empty_but_one", "ragged", "ragged_concatenated"])
def test_segments(orc, name):
    """every case with the concatenated input and through the table of one source pointer per segment"""
    case = bc.get(name)
    for flags in (0, bc.SRC_POINTERS):
        check(orc, case, _probe(case, flags), f"{name} flags={flags}")


@pytest.mark.parametrize("name", ["faces_identity", "faces_small_rotation", "faces_large_translation", "zero_sign", "edge_accepted_plus", "edge_accepted_minus",
                                  "edge_refused_plus", "edge_refused_minus", "bad_nan_sampled", "bad_nan_unsampled", "bad_inf_sampled", "bad_inf_unsampled"])
def test_faces_signs_and_poses(orc, name):
    check(orc, bc.get(name), _probe(bc.get(name)))


@_family("pass_through")
def test_pass_through(orc, name):
    check(orc, bc.get(name), _probe(bc.get(name)))


def test_every_case_is_run():
    ran = {k for k in bc.NAMES if k.startswith(("ns_", "large_", "passes_", "nseg_", "pass_through"))}
    ran |= {"collide_alternating_empty", "straddle_inside_workgroup", "straddle_at_256", "bucket_counts", "one_voxel_4096", "one_voxel_4097", "run_edges",
            "empties_lead_mid_trail", "all_empty_but_one", "ragged", "ragged_concatenated", "faces_identity", "faces_small_rotation",
            "faces_large_translation", "zero_sign", "edge_accepted_plus", "edge_accepted_minus", "edge_refused_plus", "edge_refused_minus",
            "bad_nan_sampled", "bad_nan_unsampled", "bad_inf_sampled", "bad_inf_unsampled"}
    assert ran == set(bc.NAMES)


def test_reuse_of_the_object(orc):
    """one object, call after call: the epoch-tagged fail word and reason words, cnt / heads reset by the next plan, buffers that grew
    for a large run serving a small one, a good run behind one that gave up"""
    seq = bc.reuse_sequence()
    assert [c.name for c in seq] == ["large_131073", "ns_513", "one_voxel_4097", "ns_513", "nseg_513", "large_131073"]
    for step, case in enumerate(seq):
        check(orc, case, _probe(case), f"step {step}: {case.name}")


def test_invalid_arguments_are_refused():
    p = np.zeros((4, 4), np.float32)
    one = bc.vm.IDENTITY[None]
    bad = [
        dict(points=p, seg_off=[0, 3, 2, 4], poses12=np.tile(one, (2, 1)), leaf_even=0.5),           # offsets that decrease
        dict(points=p, seg_off=[0, 3], poses12=one, leaf_even=0.5),                                  # offsets that do not end at n
        dict(points=p, seg_off=[1, 4], poses12=one, leaf_even=0.5),                                  # ... or do not start at 0
        dict(points=p, seg_off=[0, 4], poses12=one, leaf_even=0.0),                                  # leaves
        dict(points=p, seg_off=[0, 4], poses12=one, leaf_even=0.5, leaf_odd=-1.0),
        dict(points=p, seg_off=[0, 4], poses12=one, leaf_even=float("nan")),
        dict(points=p[:0], seg_off=[0, 0], poses12=one, leaf_even=0.5),                              # outside VoxBucket::fits: no point,
        dict(points=p, seg_off=[0] * 4097 + [4], poses12=np.tile(one, (2049, 1)), leaf_even=0.5),    # 4097 segments
        dict(points=p, seg_off=[0, 4], poses12=one, leaf_even=0.5, flags=2),                         # an unknown flag
    ]
    for kw in bad:
        with pytest.raises(loamx.LoamxError) as e:
            loamx.voxbucket_probe(**kw)
        assert e.value.code == loamx.E_INVALID, kw["seg_off"][:4]
    L, C = loamx.lib(), loamx.C
    assert L.loamx_voxbucket_probe(None, C.c_uint32(4), None, C.c_uint32(1), None, C.c_float(0.5), C.c_float(0.5), C.c_uint32(0), None, None, None, None,
                                   None, None, None, C.c_uint32(1)) == loamx.E_INVALID
    # far and non-finite coordinates are NOT refused: they are the stage's own give-up (test_faces_signs_and_poses)
    got = loamx.voxbucket_probe(p, [0, 4], one, 0.5)
    assert got["gave_up"] == 0 and got["out_off"][-1] == 1
