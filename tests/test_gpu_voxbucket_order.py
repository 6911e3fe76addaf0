"""GPU: the order the bucketed voxel grid works in (csrc/voxbucket.hip through loamx_voxbucket_probe): bucket words and chunk ranges
from k_vb_stack, every bucket of k_vb_reduce collecting its points in input order, a stable sort on the voxel bits alone — at the
cases of tests/voxbucket_order_cases.py, with the rule of tests/test_gpu_voxbucket_probe.py: bit for bit against the model and
pcl::VoxelGrid as the oracle restates it on the model's stack.  And the sweep set-up k_vb_plan does on the way (VbPoseInit) against
k_pose_init's, through loamx.Batch with and without LOAMX_VOX_LEGACY."""
import numpy as np
import pytest

import voxbucket_order_cases as oc
from loam_velodyne_amd import loamx, synth
from test_gpu_voxbucket_probe import check, _probe

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", oc.NAMES)
def test_order_cases(orc, name):
    check(orc, oc.get(name), _probe(oc.get(name)))


def test_sum_order_is_the_same_every_time(orc):
    """the mean of the order-dependent voxel is the sequential float32 sum in input order, run after run"""
    case = oc.get("sum_order")
    outs = []
    for _ in range(3):
        got = _probe(case)
        check(orc, case, got)
        outs.append(got["out"].tobytes())
    assert outs[0] == outs[1] == outs[2]
    out = np.frombuffer(outs[0], np.float32).reshape(-1, 4)
    row = out[out[:, 0] >= 20.0]
    assert len(row) == 1 and row[0, 3] == np.float32(0.125)


def _run(cm, sm, cl, sl, guesses):
    b = loamx.Batch(len(cl))
    b.set_frozen(cm, sm)
    b.upload(cl, sl, guesses)
    assert b.run() == loamx.OK
    poses, stats = b.download()
    return poses, stats, [b.download_ds(k) for k in range(len(cl))]


@pytest.mark.parametrize("shape", ["one", "two", "three_middle_empty"])
def test_the_plan_sets_the_sweeps_up_as_k_pose_init_does(monkeypatch, shape):
    """tiny clouds cut from the map itself; the guesses differ per sweep, so a sweep set up from another one's guess shows"""
    rng = np.random.default_rng(7)
    world = synth.World(half_extent=40.0)
    cm, sm = world.make_map(20000)
    nsw = {"one": 1, "two": 2, "three_middle_empty": 3}[shape]
    cl = [cm[rng.choice(len(cm), 300, replace=False)].copy() for _ in range(nsw)]
    sl = [sm[rng.choice(len(sm), 900, replace=False)].copy() for _ in range(nsw)]
    if shape == "three_middle_empty":
        cl[1], sl[1] = cl[1][:0], sl[1][:0]
    guesses = np.concatenate([rng.normal(0, 0.01, (nsw, 3)), rng.normal(0, 0.05, (nsw, 3))], axis=1)
    monkeypatch.delenv("LOAMX_VOX_LEGACY", raising=False)
    p0, s0, d0 = _run(cm, sm, cl, sl, guesses)
    monkeypatch.setenv("LOAMX_VOX_LEGACY", "1")
    p1, s1, d1 = _run(cm, sm, cl, sl, guesses)
    assert np.array_equal(np.asarray(p0).view(np.uint8), np.asarray(p1).view(np.uint8)) and np.array_equal(s0, s1)
    for a, b in zip(d0, d1):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert all(len(a[0]) and len(a[1]) for k, a in enumerate(d0) if len(cl[k]))   # (the clouds are not trivially empty)
