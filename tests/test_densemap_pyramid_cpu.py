"""CPU: the dense map's coarser levels and the coarse-to-fine alignment (include/loamx.h, loamx_densemap_coarsen ...
loamx_densemap_align_pyramid) — the new symbols declared and exported, the struct laid out as the binding lays it out, refusals that
need no device, and the model (tests/densemap_pyramid_model.py) against what defines it: on dyadic points the cascade's levels are,
word for word, the maps a coarser model builds; on general points a parent holds its children's points, under their halved indices, at
the n-weighted mean of their positions within the bound the model's docstring derives; and the reason the feature exists — in the box
scene at leaf 0.25 a start 1.5 m and 0.2 rad off is beyond the single loop and inside the pyramid's basin."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
import densemap_align_model as am
import densemap_model as dm
import densemap_moments_model as mm
import densemap_pyramid_model as pm
from loam_velodyne_amd import loamx

NEW_SYMBOLS = ("loamx_densemap_pyramid_default_config", "loamx_densemap_coarsen", "loamx_densemap_freeze_pyramid",
               "loamx_densemap_frozen_levels", "loamx_densemap_align_select_level", "loamx_densemap_align_pyramid",
               "loamx_densemap_align_pyramid_from_map", "loamx_densemap_align_pyramid_from_pipeline")


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    L = loamx.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    assert "#define LOAMX_PYRAMID_MAX_LEVELS 6" in hdr and loamx.PYRAMID_MAX_LEVELS == pm.MAX_LEVELS == 6
    assert L.loamx_abi_version() == 6   # additive: the ABI number stays
    for name in ("coarsen", "freeze_pyramid", "select_level", "align_pyramid", "align_pyramid_from", "align_pyramid_from_pipeline"):
        assert callable(getattr(loamx.DenseMap, name)), name
    assert isinstance(loamx.DenseMap.frozen_levels, property)
    # the expressions of the cascade stand in the header as the model restates them
    for line in ("S'_a  += (S_a >> 1) + n * b_a * 2^19",
                 "M'_ab += (M_ab >> 2) + b_a * 2^18 * S_b + b_b * 2^18 * S_a + n * b_a * b_b * 2^38"):
        assert line in hdr, line


def test_config_defaults_and_layout():
    c = loamx.PyramidConfig()
    c.levels, c.max_curvature = 99, -1.0
    loamx.lib().loamx_densemap_pyramid_default_config(C.byref(c))
    assert (c.levels, c.max_curvature) == (3, 0.0) and C.sizeof(c) == 8
    loamx.lib().loamx_densemap_pyramid_default_config(None)   # tolerated


def test_refusals_without_a_device():
    L = loamx.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    keys, vals, mom, n = np.full(2, 5, np.uint64), np.full(8, 5, np.uint64), np.full(18, 5, np.uint64), C.c_uint64(7)
    assert L.loamx_densemap_coarsen(None, C.c_uint32(1), None, ptr(keys), ptr(vals), ptr(mom), C.c_uint64(2), C.byref(n)) == loamx.E_INVALID
    assert L.loamx_densemap_freeze_pyramid(None, None, None, None, None) == loamx.E_INVALID
    levels = C.c_uint32(9)
    assert L.loamx_densemap_frozen_levels(None, C.byref(levels)) == loamx.E_INVALID
    assert L.loamx_densemap_align_select_level(None, C.c_uint32(0)) == loamx.E_INVALID
    assert "NULL argument: h" in L.loamx_last_error().decode()
    cloud = loamx.cloud_of(np.zeros((4, 4), np.float32))
    pose, out = np.eye(3, 4).reshape(12).copy(), (loamx.AlignResult * 6)()
    assert L.loamx_densemap_align_pyramid(None, C.byref(cloud), ptr(pose), None, None, C.c_uint32(0), out) == loamx.E_INVALID
    assert L.loamx_densemap_align_pyramid_from_map(None, None, ptr(pose), None, C.c_uint32(0), out) == loamx.E_INVALID
    assert L.loamx_densemap_align_pyramid_from_pipeline(None, None, C.c_uint32(0), ptr(pose), None, C.c_uint32(0), out) == loamx.E_INVALID
    assert np.all(keys == 5) and np.all(vals == 5) and np.all(mom == 5) and n.value == 7 and levels.value == 9
    assert bytes(out) == bytes(C.sizeof(out))


def test_coarsen_once_by_hand():
    # two children of one parent on x (indices -1 and -2 -> -1), one point each, and a third voxel alone under another parent
    q = {(-1, 0, 0): [(1000, 2000, 3000)], (-2, 0, 0): [(7, 9, 11)], (3, -5, 1 - (1 << 20)): [(1 << 19, 5, (1 << 20) - 1)]}
    keys, vals, mom = [], [], []
    for idx in sorted(q, key=pm.key_of):
        v, m = mm.words_of_q(q[idx], [(-3, 4, 5)])
        keys.append(pm.key_of(idx)); vals.append(v); mom.append(m)
    k1, v1, m1 = pm.coarsen_once(np.array(keys, np.uint64), np.array(vals, np.uint64), np.array(mom, np.uint64))
    assert k1.tolist() == sorted([pm.key_of((-1, 0, 0)), pm.key_of((1, -3, -(1 << 19)))])
    pos = k1.tolist().index(pm.key_of((-1, 0, 0)))
    # index -1 is the upper half of parent -1 (b = 1), index -2 its lower half; y and z: b = 0
    qa, qb = (1000 // 2 + (1 << 19), 1000, 1500), (3, 4, 5)
    assert v1[pos].tolist() == [2, qa[0] + qb[0], qa[1] + qb[1], qa[2] + qb[2]]
    assert m1[pos, 0] == qa[0] * qa[0] + (7 * 7 >> 2)    # the floor is taken on the child's word: 49 >> 2 = 12, not 3 * 3
    assert m1[pos, 3] == qa[0] * qa[1] + (7 * 9 >> 2)
    assert m1[pos, 6:].astype(np.int64).tolist() == [-6, 8, 10]
    other = 1 - pos
    assert pm.indices_of(k1[other]) == [1, -3, -(1 << 19)] and v1[other, 0] == 1
    # 3 -> b 1, -5 -> b 1, 1 - 2^20 -> b 1: every offset lands in the upper half, below 2^20
    assert v1[other, 1:].tolist() == [(1 << 18) + (1 << 19), 2 + (1 << 19), ((1 << 20) - 1 >> 1) + (1 << 19)]
    assert int(v1[other, 1:].max()) < 1 << 20


@pytest.fixture(scope="module")
def dyadic():
    pts = pm.dyadic_cloud()
    assert len(pts) == 3000
    m = mm.MomentsModel(leaf=pm.DYADIC_LEAF)
    assert m.add(pts, pm.DYADIC_ORIGIN)
    return pts, m


def test_dyadic_levels_are_the_coarser_maps(dyadic):
    pts, m = dyadic
    idx = np.array([pm.indices_of(k) for k in m.keys.tolist()])
    assert idx.min() < -30 and idx.max() > 30
    levels = pm.cascade(m.keys, m.vals, m.moments(), 3)
    for l, (keys, vals, mom) in enumerate(levels, start=1):
        c = mm.MomentsModel(leaf=pm.DYADIC_LEAF * 2 ** l)
        assert c.add(pts, pm.DYADIC_ORIGIN)
        assert keys.tolist() == c.keys.tolist(), l
        assert vals.tolist() == c.vals.tolist(), l
        assert mom.tolist() == c.moments().tolist(), l
        assert len(keys) < len(m.keys)


@pytest.fixture(scope="module")
def box():
    S = am.box_scene()
    m = mm.MomentsModel(leaf=pm.BASIN_LEAF)
    for p, o in S["sweeps"]:
        assert m.add(p, o)
    S["model"] = m
    S["levels"] = pm.cascade(m.keys, m.vals, m.moments(), 3)
    return S


def test_general_points_parents_hold_their_children(box):
    m = box["model"]
    leaf0 = pm.level_leaf(pm.BASIN_LEAF, 0)
    pos0 = dm.export(m.keys, m.vals, leaf0).astype(np.float64)
    anc = np.array([pm.indices_of(k) for k in m.keys.tolist()])    # the level-0 voxels' ancestors, level by level
    ck, cv = m.keys, m.vals
    worst = 0.0
    for l, (keys, vals, mom) in enumerate(box["levels"], start=1):
        # every parent key is its children's >> 1, and it holds their points
        child_idx = np.array([pm.indices_of(k) for k in ck.tolist()])
        parent = np.array([pm.key_of(i) for i in (child_idx >> 1).tolist()], np.uint64)
        assert sorted(set(parent.tolist())) == keys.tolist()
        where = np.searchsorted(keys, parent)
        n_sum = np.zeros(len(keys), np.uint64)
        np.add.at(n_sum, where, cv[:, 0])
        assert n_sum.tolist() == vals[:, 0].tolist()
        assert np.all(vals[:, 1:] < (vals[:, :1] << np.uint64(dm.QBITS)))    # offsets below 2^20
        # its position: the n-weighted f64 mean of the level-0 positions below it, short by less than the bound, never above
        anc = anc >> 1
        akey = np.array([pm.key_of(i) for i in anc.tolist()], np.uint64)
        at = np.searchsorted(keys, akey)
        assert np.all(keys[at] == akey)
        w = m.vals[:, 0].astype(np.float64)
        mean = np.zeros((len(keys), 3))
        np.add.at(mean, at, pos0[:, :3] * w[:, None])
        mean /= vals[:, :1].astype(np.float64)
        leaf_l = pm.level_leaf(pm.BASIN_LEAF, l)
        got = dm.export(keys, vals, leaf_l).astype(np.float64)[:, :3]
        rounding = float(np.spacing(np.float32(np.abs(pos0[:, :3]).max())))
        bound = pm.position_bound(leaf_l, vals[:, :1].astype(np.float64))
        short = mean - got
        worst = max(worst, float((short / bound).max()))
        assert np.all(short <= bound + rounding) and np.all(short >= -rounding), l
        ck, cv = keys, vals
    print(f"largest shortfall against its bound: {worst:.3f}")



def _tables(S, levels=3, max_curvature=0.0):
    m = S["model"]
    tables = [am.frozen_of(m.keys, m.surfels()[0])]
    for l in range(1, levels):
        keys, vals, mom = S["levels"][l - 1]
        tables.append(pm.frozen_of_level(keys, pm.surfels_of_level(pm.level_leaf(pm.BASIN_LEAF, l), keys, vals, mom), max_curvature))
    return tables


def test_the_basin_case(box):
    truth, leaf = box["truth"], pm.BASIN_LEAF
    start = pm.basin_start(truth)
    tables = _tables(box)
    single = am.align(*tables[0], box["cloud"], start, leaf)
    rot_s, trans_s = am.pose_error(single["pose"], truth)
    res = pm.align_pyramid(tables, box["cloud"], start, leaf)
    rot, trans = am.pose_error(res[-1]["pose"], truth)
    print(f"single level: status {single['status']}, {single['iterations']} iterations, {rot_s:.3e} rad, {trans_s:.3e} m; pyramid: status "
          f"{[r['status'] for r in res]}, iterations {[r['iterations'] for r in res]}, {rot:.3e} rad, {trans:.3e} m")
    assert trans_s > leaf    # the single loop does not reach the truth
    assert len(res) == 3 and rot <= 0.01 and trans <= leaf / 10
    assert all(r["status"] == 0 for r in res)
    # each level starts where the level before ended
    again = am.align(*tables[1], box["cloud"], res[0]["pose"], pm.level_leaf(leaf, 1))
    assert again["pose"].tobytes() == res[1]["pose"].tobytes()


def test_a_level_that_matches_too_little_hands_its_input_on(box):
    tables = _tables(box, 2)
    start = pm.basin_start(box["truth"])
    res = pm.align_pyramid(tables, box["cloud"][:300], start, pm.BASIN_LEAF, min_matched=301)
    assert [r["status"] for r in res] == [2, 2] and res[0]["pose"].tobytes() == start.tobytes() == res[1]["pose"].tobytes()
