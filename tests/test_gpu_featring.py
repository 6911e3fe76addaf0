"""GPU: the order-dependent picks of k_feat_ring (csrc/features.hip) against the oracle's ScanRegistration, word for word (clouds
compared as uint32 words, no tolerance anywhere), on the designed rings of tests/featring_cases.py: equal curvatures, a curvature
exactly at the threshold, walks that skip whole rounds of 64 candidates, every event of the settlement between regions, the double
comparisons on their constants, the edges of the occlusion mask, gap breaks of markAsPicked, the ring's start in the sweep, the sort
networks on both sides of every switch with adversarial content, and all of it mixed in one batch.

tests/test_featring_cases_cpu.py proves each case the edge it claims to be and the model, the oracle and the compiled reference equal
on all of them; tests/test_gpu_tests_dry_run.py runs the bodies below on the CPU over the oracle-backed test double.  A failure
names the case, the first differing row, the point it came from, that point's region as analyse() sees it, and the claim."""
import numpy as np
import pytest

import featring_cases as fc
import oracle_py as op
from loam_velodyne_amd import loamx, synth

pytestmark = pytest.mark.gpu

CASES = fc.cases()
ANALYSIS = {}


def _analysis(case):
    if case.name not in ANALYSIS:
        ANALYSIS[case.name] = fc.analyse(case)
    return ANALYSIS[case.name]


def process(case, handle=None):
    if handle is None:
        handle = loamx.ScanRegistration(**case.device_config())
    else:
        handle.configure(**case.device_config())
    return handle.process(case.cloud(), case.sizes())


def explain(case, got, want, where=""):
    """None when the four clouds are equal word for word; otherwise the message that names the path"""
    d = fc.first_difference(got, want)
    if d is None:
        return None
    name, row = d
    g = got[name][row] if row < len(got[name]) else None
    w = want[name][row] if row < len(want[name]) else None
    ring, index = fc.source_of(w if w is not None else g)
    a = _analysis(case)
    region = fc.describe_region(fc.region_of(case, ring, index, a)) if ring < len(a) and a[ring]["processed"] else "ring not processed"
    path = "side by side" if ring < len(a) and a[ring]["simple"] else "sequential walk"
    msg = (f"{case.name}{where}: cloud `{name}` row {row}: device {g} != oracle {w} ({len(got[name])} / {len(want[name])} rows); source ring {ring} "
           f"point {index} ({path}, sortP {a[ring]['sortP'] if ring < len(a) else '?'}); {region}; written for {case.claims}")
    print(msg)
    return msg


def check_case(orc, case, handle=None, where=""):
    got = process(case, handle)
    msg = explain(case, got, fc.cached_oracle(orc, case), where)
    assert msg is None, msg
    return got


def check_handle_reuse(orc):
    seq = [fc.by_name(n, CASES) for n in fc.REUSE_ORDER]
    handle = loamx.ScanRegistration(**seq[0].device_config())
    results = []
    for step, case in enumerate(seq):
        got = check_case(orc, case, handle, f" (step {step} of one handle)")
        fresh = process(case)
        assert fc.first_difference(got, fresh) is None, (step, case.name, fc.first_difference(got, fresh))
        results.append(got)
    assert fc.first_difference(results[0], results[-1]) is None


def _rows_of_ring(cloud, ring):
    return cloud[np.floor(cloud[:, 3]) == ring]


def check_start_index(orc):
    """the designed ring behind fillers of 0 to 13 points.  The region formula's floor does not depend on the ring's start (see
    tests/featring_cases.py), so the designed ring's picks are the SAME rows at every offset — and there are picks to compare."""
    fam = [c for c in CASES if c.name.startswith("start index")]
    assert len(fam) == len(fc.START_OFFSETS)
    rows = []
    for case in fam:
        got = check_case(orc, case)
        rows.append({n: _rows_of_ring(got[n], case.claims["designed"]) for n in fc.NAMES})
    assert len(rows[0]["sharp"]) >= 8 and len(rows[0]["flat"]) >= 12 and len(rows[0]["less_flat"]) >= 250
    for case, r in zip(fam[1:], rows[1:]):
        assert fc.first_difference(r, rows[0]) is None, case.name


def check_mixed_batch(orc):
    case = fc.by_name("mixed batch", CASES)
    got = check_case(orc, case)
    per_ring = [len(_rows_of_ring(got["less_flat"], r)) for r in range(len(case.rings))]
    assert per_ring[1] == per_ring[2] == per_ring[6] == 0 and min(per_ring[0], per_ring[3], per_ring[4], per_ring[5]) > 0


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case(orc, case):
    check_case(orc, case)


def test_handle_reuse(orc):
    check_handle_reuse(orc)


def test_start_index(orc):
    check_start_index(orc)


def test_mixed_batch(orc):
    check_mixed_batch(orc)


def _designed_sweep(names, filler, shift):
    """the designed rings of the named cases (six regions, curvature region 5) in front of an ordinary sweep's rings"""
    rings = [fc.restamp(fc.by_name(n, CASES).rings[0], r) for r, n in enumerate(names)]
    pts = filler.points.copy()
    pts[:, 3] += np.float32(shift)
    return np.concatenate(rings + [pts]), [len(r) for r in rings] + list(filler.ring_sizes)


def test_pipeline_base(orc, small_world):
    """streams 1 and 2 of a three-stream Pipeline carry designed rings (stream 0 an ordinary sweep), so their rings start far from 0 in
    the batch's cloud and ring_sweep_base != 0.  After step 0 nothing has been re-projected: the stream's last corner and surface
    clouds are the sweep's less-sharp and less-flat clouds, and equal the oracle odometry's for the oracle's features word for word.
    The leaf is the default 0.2 m here: at the cases' 2^-9 an ordinary sweep spans more than INT_MAX voxels, pcl::VoxelGrid copies it
    through, and a -0.0 coordinate comes out as +0.0 on the device (the difference csrc/voxel.hpp documents)."""
    cm, sm = small_world.make_map(30000)
    move = np.array([0.002, 0.02, -0.001, 0.2, 0.01, 0.8])
    sw = [synth.make_sweep(small_world, "VLP-16", np.zeros(6), move, seed=70 + k, az_steps=600) for k in range(3)]
    cfg = fc.by_name("settlement, cascade", CASES)
    names = (("settlement, cascade", "settlement, mark withdrawn", "gap break on a region boundary", "settlement, one region remade"),
             ("settlement, mark added", "picks at the ring's first and last region point", "settlement, marks on unpicked points only"))
    for n in names[0] + names[1]:
        assert fc.by_name(n, CASES).nreg == cfg.nreg and fc.by_name(n, CASES).cr == cfg.cr
    data = [(sw[0].points, list(sw[0].ring_sizes)), _designed_sweep(names[0], sw[1], len(names[0])), _designed_sweep(names[1], sw[2], len(names[1]))]
    dcfg, ocfg = dict(cfg.device_config(), less_flat_filter_size=0.2), dict(cfg.oracle_config(), lessFlatFilterSize=0.2)
    p = loamx.Pipeline(3, scanreg=dcfg)
    p.set_frozen(cm, sm)
    for s in range(3):
        p.set_state(s, aft=np.zeros(6, np.float32))
    p.upload([data])
    p.step(0)
    for k in range(3):
        gc, gs = p.last_clouds(k, len(data[k][0]))
        ood = op.LaserOdometry(orc)
        ood.set_features(op.ScanRegistration(orc, **ocfg).process(*data[k]))
        ood.process()
        oc, os_ = ood.last_corner(), ood.last_surf()
        assert len(oc) > 100 and len(os_) > 1000
        if k:   # the designed rings (ring numbers below the filler's) have picks in the clouds compared
            assert (np.floor(oc[:, 3]) < len(names[k - 1])).sum() >= 6 and (np.floor(os_[:, 3]) < len(names[k - 1])).sum() >= 20
        for what, g, o in (("last corner", gc, oc), ("last surf", gs, os_)):
            assert g.shape == o.shape, (k, what, g.shape, o.shape)
            bad = np.flatnonzero((g.view(np.uint32) != o.view(np.uint32)).any(axis=1))
            assert not len(bad), (k, what, int(bad[0]), g[bad[0]], o[bad[0]], fc.source_of(o[bad[0]]))
