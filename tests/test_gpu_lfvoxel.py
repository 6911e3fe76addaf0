"""GPU: the per-ring less-flat voxel grid (csrc/features.hip: k_feat_lf_voxel; the generic VoxelPipeline for rings of more than 4096
points) against pcl::VoxelGrid as the oracle restates it, bit for bit (clouds compared as uint32 words), at the shapes whole sweeps
never reach: 0 to 4 radix passes, pass-through, one voxel, runs across the 1024-thread steps, every per_wave, points on voxel faces,
skewed digit histograms, mixed batches, the 4096 / 4097 dispatch boundary, one handle reused across very different calls, and the
linked (split hand-over) path at three leaves.

The kernel is driven through the public ScanRegistration.process: with surface_curvature_threshold = 3e38 every region point is a
less-flat candidate and nothing is a corner (tests/lfvoxel_cases.py; tests/test_lfvoxel_cases_cpu.py proves each case the edge it
claims to be and the premise against the oracle's full ScanRegistration).  tests/test_gpu_tests_dry_run.py runs the bodies below on
the CPU over the oracle-backed test double."""
import numpy as np
import pytest

import lfvoxel_cases as lc
import oracle_py as op
from loam_velodyne_amd import loamx, synth

pytestmark = pytest.mark.gpu

CASES = lc.all_cases()


def process(case, handle=None):
    if handle is None:
        handle = loamx.ScanRegistration(**case.device_config())
    else:
        handle.configure(**case.device_config())
    return handle.process(case.cloud(), case.sizes())


def compare(case, got, want, where=""):
    """got: the clouds of process(); want: (reference cloud, per-ring offsets)"""
    ref, off = want
    out = got["less_flat"]
    what = f"{case.name}{where}"
    a, b = out.view(np.uint32), ref.view(np.uint32)
    k = min(len(a), len(b))
    bad = np.flatnonzero((a[:k] != b[:k]).any(axis=1))
    if len(bad):
        row = int(bad[0])
        ring = int(np.searchsorted(off, row, side="right") - 1)
        print(f"{what}: {len(bad)} of {k} rows differ, first row {row} = ring {ring}, its voxel {row - int(off[ring])}: {out[row]} != {ref[row]}")
    assert out.shape == ref.shape, f"{what}: {out.shape} != {ref.shape}"
    assert not len(bad), what
    assert len(got["sharp"]) == 0 and len(got["less_sharp"]) == 0, what


def check_case(orc, case):
    compare(case, process(case), lc.cached_reference(orc, case))


def check_dispatch_boundary(orc):
    short, long_ = lc.dispatch_pair()
    assert short.sizes() == [lc.LFV_MAX] and long_.sizes() == [lc.LFV_MAX + 1]
    g_short, g_long = process(short), process(long_)
    compare(short, g_short, lc.cached_reference(orc, short))
    compare(long_, g_long, lc.cached_reference(orc, long_))
    assert np.array_equal(g_short["less_flat"].view(np.uint32), g_long["less_flat"].view(np.uint32))
    mixed = lc.mixed_batch_case(longest=lc.LFV_MAX + 1)   # every ring of the batch through the generic pipeline
    assert max(mixed.sizes()) == lc.LFV_MAX + 1
    compare(mixed, process(mixed), lc.cached_reference(orc, mixed))


def check_handle_reuse(orc):
    seq = [lc.by_name(n, CASES) for n in lc.REUSE_ORDER]
    handle = loamx.ScanRegistration(**seq[0].device_config())
    results = []
    for step, case in enumerate(seq):
        got = process(case, handle)
        fresh = process(case)
        for name in loamx.ScanRegistration.NAMES:
            assert got[name].shape == fresh[name].shape and np.array_equal(got[name].view(np.uint32), fresh[name].view(np.uint32)), (step, case.name, name)
        compare(case, got, lc.cached_reference(orc, case), f" (step {step} of one handle)")
        results.append(got["less_flat"])
    assert np.array_equal(results[0].view(np.uint32), results[-1].view(np.uint32))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case(orc, case):
    check_case(orc, case)


def test_dispatch_boundary(orc):
    check_dispatch_boundary(orc)


def test_handle_reuse(orc):
    check_handle_reuse(orc)


@pytest.mark.parametrize("leaf", [0.05, 0.2, 2.0])
def test_linked_path(orc, small_world, leaf):
    """run_async's split hand-over (host-mirrored offsets, the less-flat cloud taken late): the first frame's last surface cloud is
    the less-flat cloud itself — nothing is re-projected — so it equals the oracle odometry's for the oracle's features byte for byte"""
    sw = synth.make_sweep(small_world, "VLP-16", np.zeros(6), np.array([0.002, 0.02, -0.001, 0.2, 0.01, 0.8]), seed=31, az_steps=600)
    sr, od = loamx.ScanRegistration(less_flat_filter_size=leaf), loamx.LaserOdometry()
    sr.process_linked(sw.points, sw.ring_sizes)
    assert od.process_linked(sr) == loamx.SKIPPED
    got = od.last_clouds()[1]
    ood = op.LaserOdometry(orc)
    ood.set_features(op.ScanRegistration(orc, lessFlatFilterSize=leaf).process(sw.points, sw.ring_sizes))
    ood.process()
    want = ood.last_surf()
    assert len(want) > 100 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
