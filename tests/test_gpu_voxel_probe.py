"""GPU: the segmented voxel grid on its own (csrc/voxel.hip: k_vox_ijk, k_vox_ds, k_vox_ds_seg through loamx_voxel_probe) against
pcl::VoxelGrid per segment as the oracle restates it — bit for bit (the clouds are compared as uint32 words: -0.0 is not 0.0), with
the output offsets, at the shapes where such kernels go wrong: sizes around the 2048-element tile, voxel runs that cross tile ends,
every key width and with it every number of sort passes, pass-through segments, points on voxel faces, empty segments, scattered
segment ids, masks, and one pipeline reused from call to call.  tests/voxel_cases.py builds the cases and
tests/test_voxel_cases_cpu.py proves that each one is the edge it claims to be.

Every case runs under the default launch, with LOAMX_VDS_WGS=1 (one workgroup walks every tile through its list) and — contiguous
unmasked input, which otherwise goes to k_vox_ds_seg — with LOAMX_VDS_GLOBAL=1 through the general kernel."""
import numpy as np
import pytest

import voxel_cases as vc
from loam_velodyne_amd import loamx

pytestmark = pytest.mark.gpu

_REF = {}


def _reference(orc, case):
    if id(case) not in _REF:
        _REF[id(case)] = (case, *vc.reference(orc, case))   # (the case is kept: its id stays its own)
    return _REF[id(case)][1:]


def _probe(case):
    return loamx.voxel_probe(case.pts, case.nseg, case.leaf_even, case.leaf_odd, seg_off=case.seg_off, seg_ids=case.seg_ids, valid=case.valid)


def _compare(case, env, got, want):
    (out, off), (ref, ref_off) = got, want
    where = f"{case.name} {env or 'default'}"
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


def check(orc, monkeypatch, case):
    want = _reference(orc, case)
    for env in case.settings():
        for k in ("LOAMX_VDS_WGS", "LOAMX_VDS_GLOBAL"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _compare(case, env, _probe(case), want)


_by_name = lambda cases: pytest.mark.parametrize("case", cases, ids=lambda c: c.name)


@_by_name(vc.tile_edge_cases())
def test_tile_edges(orc, monkeypatch, case):
    check(orc, monkeypatch, case)


@_by_name(vc.run_cases())
def test_runs_across_tiles(orc, monkeypatch, case):
    check(orc, monkeypatch, case)


@pytest.mark.parametrize("B", vc.KEY_BITS)
def test_key_width_and_passes(orc, monkeypatch, B):
    for case in vc.key_width_cases(B):
        check(orc, monkeypatch, case)


@_by_name(vc.passthrough_cases())
def test_pass_through(orc, monkeypatch, case):
    want = _reference(orc, case)
    seg, ok = case.seg_of_point(), case.valid_mask()
    for s in case.claims["passthrough"]:   # (the reference itself: the segment's input in input order)
        assert np.array_equal(want[0][want[1][s]:want[1][s + 1]].view(np.uint32), case.pts[ok & (seg == s)].view(np.uint32))
    check(orc, monkeypatch, case)


@_by_name(vc.face_cases())
def test_faces_and_signs(orc, monkeypatch, case):
    check(orc, monkeypatch, case)


@pytest.mark.parametrize("nseg", vc.SEGMENT_NSEG)
def test_segments(orc, monkeypatch, nseg):
    for case in vc.segment_cases(nseg):
        check(orc, monkeypatch, case)


@_by_name(vc.mask_cases())
def test_mask(orc, monkeypatch, case):
    check(orc, monkeypatch, case)
    if not case.valid_mask().any():
        out, off = _probe(case)
        assert len(out) == 0 and not off.any()


def test_reuse_of_the_pipeline(orc, monkeypatch):
    """one pipeline, call after call: its cleared block is laid out per (n, nseg), grows, and is prepared by the index kernel only
    for the general kernel that follows — every call of the sequence must equal the reference"""
    for k in ("LOAMX_VDS_WGS", "LOAMX_VDS_GLOBAL"):
        monkeypatch.delenv(k, raising=False)
    seq = vc.reuse_sequence()
    assert [c.name for c in seq] == ["reuse_large_general", "reuse_small_segmented", "reuse_large_general", "reuse_n0", "reuse_nseg5000", "reuse_nseg1"]
    for step, case in enumerate(seq):
        _compare(case, {"step": step}, _probe(case), _reference(orc, case))


def test_invalid_arguments_are_refused():
    p = np.zeros((4, 4), np.float32)
    with pytest.raises(loamx.LoamxError) as e:
        loamx.voxel_probe(p, 2, 0.5, seg_ids=[0, 1, 2, 0])       # segment id beyond nseg
    assert e.value.code == loamx.E_INVALID
    with pytest.raises(loamx.LoamxError) as e:
        loamx.voxel_probe(p, 2, 0.5, seg_off=[0, 3, 2])          # offsets that do not end at n
    assert e.value.code == loamx.E_INVALID
    with pytest.raises(loamx.LoamxError) as e:
        loamx.voxel_probe(p, 1, 0.5)                             # neither seg_off nor seg_ids
    assert e.value.code == loamx.E_INVALID
    with pytest.raises(loamx.LoamxError) as e:
        loamx.voxel_probe(p, 1, 0.0, seg_off=[0, 4])             # leaf
    assert e.value.code == loamx.E_INVALID
